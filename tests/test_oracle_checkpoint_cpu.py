"""CPU: oracle/sr_oracle.py's checkpointed forward (sr_forward_checkpointed, the float64 yardstick of the full-size training
steps in tests/test_full_size_f64_gpu.py) computes the same training step as the plain oracle: output, loss, every parameter
gradient, the stage gradients and the BatchNorm buffers after the forward, in float64."""
import torch
import torch.nn.functional as F

from oracle import sr_oracle, synth


def _rel(a, b):
    """max-normalised difference; 0 for two all-zero tensors (a dead ReLU unit of the tiny network)"""
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-300)).item()


def test_checkpointed_training_step_equals_the_plain_oracle():
    Fc, N, win, s, B, H, W = 16, 2, 1, 2, 2, 24, 40
    sd = synth.formula_state(3, s, Fc, N, win, gain=synth.GOLDEN_GAIN)
    x = synth.formula_clip(B, 2 * win + 1, H, W, seed=5).double()
    tgt = synth.formula_target(B, H * s, W * s, seed=6).double()

    ora = sr_oracle.OracleSR(3, s, Fc, N, win).double()
    ora.load_named(sd)
    ora.train()
    out, inter = ora(x, return_intermediate=True)
    keep = [inter["aggregated"], inter["residual"], inter["fused"], *inter["features"], *inter["flows"].values()]
    for v in keep:
        v.retain_grad()
    loss = F.mse_loss(out, tgt)
    loss.backward()
    bufs = {n: ora.named()[n].detach().clone() for n in ora._bufs}

    ck = sr_oracle.OracleSR(3, s, Fc, N, win).double()
    ck.load_named(sd)
    P = ck.P()
    out_c, inter_c = sr_oracle.sr_forward_checkpointed(P, x, training=True)
    keep_c = [inter_c["aggregated"], inter_c["residual"], inter_c["fused"], *inter_c["features"], *inter_c["flows"].values()]
    for v in keep_c:
        v.retain_grad()
    snap = {n: P[n].detach().clone() for n in ck._bufs}
    loss_c = F.mse_loss(out_c, tgt)
    loss_c.backward()

    assert _rel(out_c.detach(), out.detach()) <= 1e-12
    assert abs(loss_c.item() - loss.item()) <= 1e-12 * loss.item()
    live = 0
    for n in ck._names:
        g, r = P[n].grad, ora.named()[n].grad
        assert g is not None, n
        assert _rel(g, r) <= 1e-12, (n, _rel(g, r))
        live += int(r.abs().max() > 0)
    assert live >= len(ck._names) - 4
    for a, b in zip(keep_c, keep):
        assert _rel(a.detach(), b.detach()) <= 1e-12 and _rel(a.grad, b.grad) <= 1e-12
    # the buffers after the forward: the one update a training step makes
    for n in ck._bufs:
        assert _rel(snap[n].double(), bufs[n].double()) <= 1e-12, n
    # ... which the backward's recompute repeats (hence the snapshot): running stats moved again, the counter bumped T more
    T = 2 * win + 1
    cnt = "feature_extractor.body.0.bn.num_batches_tracked"
    assert int(P[cnt]) == int(snap[cnt]) + T
    assert not torch.equal(P["feature_extractor.body.0.bn.running_mean"], snap["feature_extractor.body.0.bn.running_mean"])
