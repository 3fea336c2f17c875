"""CPU: the layer of nerve_cl/_bucket.py that the flat-bucket consumers share - grad_alias_mask, Segment / segments_of, flat_grad,
grad_pairs, the data-parallel refusal - on a SuperResolutionNet put into the aliasing state by hand (no backward runs on the CPU):
every ``.grad`` is made the view of a fresh gradient bucket, which is then declared the network's last one."""
import subprocess
import sys

import pytest
import torch

import nerve_cl.ops
from nerve_cl import parallel
from nerve_cl._bucket import Segment, flat_grad, grad_pairs, refuse_loose_gradients, segments_of
from nerve_cl.models import EnhancementConfig, EnhancementEngine, SuperResolutionNet


def _aliasing_net():
    net = SuperResolutionNet(3, 2, 16, 1, 1)
    flat, views = net._new_grad_bucket()
    flat.copy_(torch.arange(flat.numel(), dtype=torch.float32))
    for n, p in net.named_parameters():
        p.grad = views[n]
    net._last_grad_bucket = flat
    return net, flat


def _engine():
    return EnhancementEngine(EnhancementConfig(frame_recovery_enabled=False, scale_factor=2, sr_num_features=16,
                                               sr_num_residual_blocks=1, sr_temporal_window=1))


def test_mask_is_all_true_in_the_aliasing_state_and_false_exactly_at_a_replaced_gradient():
    net, _ = _aliasing_net()
    names = [n for n, _ in net.named_parameters()]
    assert net.grad_alias_mask() == [True] * 47
    for k in (0, 20, 46):
        p = net.get_parameter(names[k])
        kept, p.grad = p.grad, p.grad.clone()
        assert net.grad_alias_mask() == [i != k for i in range(47)]
        p.grad = None
        assert net.grad_alias_mask() == [i != k for i in range(47)]
        p.grad = kept
    assert all(net.grad_alias_mask())


def test_mask_is_none_without_a_usable_bucket():
    net, flat = _aliasing_net()
    for bucket in (None, flat[:-4], torch.cat([flat, flat[:4]]), flat.double()):
        net._last_grad_bucket = bucket
        assert net.grad_alias_mask() is None
    net._last_grad_bucket = flat
    assert all(net.grad_alias_mask())
    assert SuperResolutionNet(3, 2, 16, 1, 1).grad_alias_mask() is None            # no backward yet


def test_grad_pairs_is_the_bucket_itself_in_the_aliasing_state():
    net, flat = _aliasing_net()
    segs = segments_of(net)
    assert len(segs) == 1 and segs[0].net is net and segs[0].aliased()
    ref = torch.zeros(segs[0].numel())
    pairs = grad_pairs(segs, [ref], "test")
    assert len(pairs) == 1
    g, r, dst = pairs[0]
    assert g is flat and r is ref and dst is None
    assert g.numel() == 320088 and sum(p.numel() for p in net.parameters()) == 320083       # the padding is part of the pair
    assert segs[0].grads() is flat


def test_grad_pairs_goes_per_parameter_once_a_gradient_left_the_bucket():
    net, flat = _aliasing_net()
    segs = segments_of(net)
    named = list(net.named_parameters())
    named[3][1].grad = named[3][1].grad.clone()
    assert not segs[0].aliased()
    ref = torch.arange(segs[0].numel(), dtype=torch.float32) * 0.5
    pairs = grad_pairs(segs, [ref], "test")
    assert len(pairs) == 47
    lay, _ = net._bucket_layout()
    for (n, p), (g, r, dst) in zip(named, pairs):
        o, k = lay[n]
        assert dst is None and g.data_ptr() == p.grad.data_ptr() and g.shape == (k,)
        assert r.data_ptr() == ref.data_ptr() + 4 * o and r.shape == (k,)
    named[5][1].grad = None
    named[7][1].grad = None
    pairs = grad_pairs(segs, None, "test")
    assert len(pairs) == 45 and all(r is None for _, r, _ in pairs)
    assert [g.data_ptr() for g, _, _ in pairs] == [p.grad.data_ptr() for _, p in named if p.grad is not None]
    gathered = segs[0].grads()                      # the same gradients in bucket layout, zeros where there is none
    assert gathered is not flat and gathered.shape == flat.shape
    for n, p in named:
        o, k = lay[n]
        assert torch.equal(gathered[o:o + k], p.grad.reshape(-1) if p.grad is not None else torch.zeros(k))


def test_flat_grad_returns_the_gradients_own_memory_or_a_copy_with_its_destination():
    g = torch.randn(6, 4)
    flat, dst = flat_grad(g)
    assert dst is None and flat.data_ptr() == g.data_ptr() and flat.shape == (24,)
    t = g.t()
    flat, dst = flat_grad(t)
    assert dst.data_ptr() == t.data_ptr() and dst.stride() == t.stride()           # the gradient itself, to copy back into
    assert flat.data_ptr() != g.data_ptr() and flat.is_contiguous() and flat.dtype == torch.float32
    assert torch.equal(flat, t.contiguous().view(-1))
    flat.mul_(2.0)
    dst.copy_(flat.view(dst.shape))                 # what a caller that changed the copy does
    assert torch.equal(g.t().contiguous().view(-1), flat)
    # a float64 gradient: on the CPU "any floating type" is taken as it is (AGEM's float64 composition on a double module); the
    # fp32 copy with dst = g is the GPU's rule, asserted in test_bucket_layer_gpu.py
    d = torch.randn(5, dtype=torch.float64)
    flat, dst = flat_grad(d)
    assert dst is None and flat.data_ptr() == d.data_ptr() and flat.dtype == torch.float64
    flat, dst = flat_grad(d.view(1, 5).expand(3, 5))
    assert dst is not None and flat.dtype == torch.float64 and flat.shape == (15,)


def test_segments_of_the_engine_and_of_a_partially_frozen_network():
    eng = _engine()
    segs = segments_of(eng)
    assert [(type(sg), sg.net is eng.super_resolution, len(sg.names)) for sg in segs] == [(Segment, True, 47), (Segment, False, 1)]
    assert segs[1].net is None and segs[1].names == ["enhancement_strength"]
    assert segs[0].names == ["super_resolution." + n for n in eng.super_resolution._param_names]
    next(eng.super_resolution.parameters()).requires_grad_(False)
    segs = segments_of(eng)                         # today's rule: a network with a frozen parameter is no segment
    assert len(segs) == 1 and segs[0].net is None and len(segs[0].names) == 47
    assert "enhancement_strength" in segs[0].names


def test_a_loose_gradient_is_refused_in_a_multi_rank_run(monkeypatch):
    eng = _engine()
    segs = segments_of(eng)
    eng.enhancement_strength.grad = torch.ones(1)
    grad_pairs(segs, None, "single")                # one rank: nothing to refuse
    monkeypatch.setattr(parallel, "world_size", lambda group=None: 2)
    with pytest.raises(RuntimeError, match=r"clip_grad_norm_: parameter 'enhancement_strength' lies outside the bucketed"):
        grad_pairs(segs, None, "clip_grad_norm_")
    with pytest.raises(RuntimeError, match=r"what: parameter 'w' lies outside.*does not synchronise such gradients"):
        refuse_loose_gradients([("v", torch.nn.Parameter(torch.ones(1))), ("w", eng.enhancement_strength)], "what", None)
    eng.enhancement_strength.grad = None
    assert grad_pairs(segs, None, "clip_grad_norm_") == []


def test_ops_does_not_import_the_continual_package():
    """``nerve_cl/__init__`` itself imports nerve_cl.continual, so the child takes ``nerve_cl`` as a bare namespace of the same
    directory: what is in sys.modules afterwards is what ops (and the modules it imports) pulled in."""
    code = ("import sys, types, os, importlib.util as u\n"
            "d = os.path.dirname(u.find_spec('nerve_cl').origin)\n"
            "pkg = types.ModuleType('nerve_cl'); pkg.__path__ = [d]; sys.modules['nerve_cl'] = pkg\n"
            "import nerve_cl.ops\n"
            "assert nerve_cl.ops.clip_grad_norm_.__module__ == 'nerve_cl.ops'\n"
            "bad = sorted(m for m in sys.modules if m.startswith('nerve_cl.continual'))\n"
            "assert not bad, bad\n"
            "print('ok', sorted(m for m in sys.modules if m.startswith('nerve_cl.')))\n")
    env_path = [p for p in sys.path if p]
    res = subprocess.run([sys.executable, "-c", "import sys; sys.path[:0] = %r\n%s" % (env_path, code)],
                         capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and res.stdout.startswith("ok"), res.stdout + res.stderr
    src = open(nerve_cl.ops.__file__).read()
    assert "nerve_cl.continual import" not in src and "import nerve_cl.continual" not in src      # no lazy import either
