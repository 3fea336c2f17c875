"""GPU: nvq_pw_bn_backward_ex / _finish with NVQ_PW_RECOMPUTE.  The backward of pointwise 1x1 -> BatchNorm -> ReLU then forms
p = bf16(d W^T) again from the d tile it stages instead of reading the p that nvq_dwpw_forward stored.  The recomputed p must
be the stored one bit for bit (one differing bit flips a ReLU mask), so every output of the flagged call is compared with
torch.equal against the call that reads p: on the d, p and statistics nvq_dwpw_forward produced, with training and eval
statistics, with a frozen BatchNorm affine (the _ex form without dgamma / dbeta) and through the reduce / finish pair of the
synchronised BatchNorm.  One of the two runs is also held against autograd of the reference ops on the stored p, at the
tolerances test_kernels_gpu.py uses for this kernel."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

C = 64
# (group_images, groups, H, W): one ragged 128-pixel tile per group, tiles cut at the group boundaries; 528 tiles = more than
# the workgroup limit, so workgroups walk several tiles and the prefetch registers rotate; groups of two images
GEOMETRIES = [(1, 3, 13, 21), (3, 1, 150, 150), (2, 3, 9, 14)]


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device")
    from nerve_cl import _nvq
    _nvq.lib()
    return _nvq


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed + sum(shape))
    return (torch.rand(*shape, generator=g) * 2 - 1) * scale


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


def nchw(t):
    return t.float().permute(0, 3, 1, 2).contiguous().cpu()


@pytest.fixture(scope="module", params=GEOMETRIES, ids=lambda g: "B%d-G%d-%dx%d" % g)
def case(request, K):
    """d, p and the batch statistics as nvq_dwpw_forward leaves them, a bf16 dy and the layer's parameters"""
    B, G, H, W = request.param
    N = B * G
    x = (rnd(N, H, W, C, seed=1) * 1.5 + 0.2).cuda().bfloat16()
    wd, wp = rnd(C, 1, 3, 3, seed=2).cuda(), rnd(C, C, 1, 1, seed=3, scale=0.15).cuda()      # fp32: the kernels round W themselves
    gamma, beta = (1 + 0.2 * rnd(C, seed=4)).cuda(), (0.1 * rnd(C, seed=5)).cuda()
    rm, rv = (0.1 * rnd(C, seed=6)).cuda(), (1 + 0.3 * rnd(C, seed=7).abs()).cuda()
    ws = torch.empty(K.wgrad_workspace_bytes() // 4 + (1 << 20), dtype=torch.float32, device="cuda")
    d, p = torch.empty_like(x), torch.empty_like(x)
    mean, invstd = torch.empty(G, C, device="cuda"), torch.empty(G, C, device="cuda")
    K.dwpw_forward(x, None, wd, wp, d, p, B, list(range(G)), mean, invstd, rm.clone(), rv.clone(), ws)
    emean, einvstd = torch.empty(G, C, device="cuda"), torch.empty(G, C, device="cuda")
    K.bn_eval_stats(rm, rv, G, emean, einvstd)
    dy = rnd(N, H, W, C, seed=8).cuda().bfloat16()
    return dict(K=K, B=B, G=G, N=N, H=H, W=W, d=d, p=p, wp=wp, gamma=gamma, beta=beta, rm=rm, rv=rv, ws=ws, dy=dy,
                stats={True: (mean, invstd), False: (emean, einvstd)})


def backward(c, training, recompute, affine=True):
    K = c["K"]
    mean, invstd = c["stats"][training]
    dd = torch.full_like(c["p"], 7.0)
    dg, db = (torch.full((C,), 7.0, device="cuda"), torch.full((C,), 7.0, device="cuda")) if affine else (None, None)
    dw = torch.full((C, C, 1, 1), 7.0, device="cuda")
    K.pw_bn_backward(c["dy"], c["p"], c["d"], c["B"], mean, invstd, c["gamma"], c["beta"], training, c["wp"], dd, dg, db, dw,
                     c["ws"], recompute=recompute)
    return dd, dw, dg, db


@pytest.mark.parametrize("training", [True, False])
def test_recomputed_p_gives_the_same_bits(case, training):
    dd0, dw0, dg0, db0 = backward(case, training, False)
    dd1, dw1, dg1, db1 = backward(case, training, True)
    assert torch.equal(dd1, dd0) and torch.equal(dw1, dw0) and torch.equal(dg1, dg0) and torch.equal(db1, db0)
    # a frozen BatchNorm affine: the _ex form without dgamma / dbeta
    dd2, dw2, _, _ = backward(case, training, True, affine=False)
    assert torch.equal(dd2, dd0) and torch.equal(dw2, dw0)
    # autograd of the reference ops (efficient_layers.py:49-66) on the stored p, per frame group
    B, G = case["B"], case["G"]
    pl = nchw(case["p"]).requires_grad_()
    gg, bg = case["gamma"].cpu().requires_grad_(), case["beta"].cpu().requires_grad_()
    outs = [F.relu(F.batch_norm(pl[g * B:(g + 1) * B], case["rm"].cpu().clone(), case["rv"].cpu().clone(), gg, bg, training,
                                0.1, 1e-5)) for g in range(G)]
    torch.cat(outs, 0).backward(nchw(case["dy"]))
    dp16 = pl.grad.bfloat16().float()                           # dp as the kernel's matrix cores see it
    w16 = case["wp"].cpu().bfloat16().float()
    dd_ref = F.conv_transpose2d(dp16, w16)
    dw_ref = torch.einsum("nohw,nihw->oi", dp16, nchw(case["d"]))
    e = (rel(nchw(dd1), dd_ref), rel(dw1.reshape(C, C), dw_ref), rel(dg1, gg.grad), rel(db1, bg.grad))
    print(f"recompute vs autograd: dd {e[0]:.3e} dweight {e[1]:.3e} dgamma {e[2]:.3e} dbeta {e[3]:.3e}")
    assert e[0] < 1.5e-2                                        # dp and dd each rounded to bf16 once
    assert e[1] < 1e-2
    assert e[2] < 1e-4 and e[3] < 1e-4


def test_recomputed_p_behind_the_synchronised_sums(case):
    """the finish phase of a synchronised BatchNorm (fp64 sums of the reduce phase, global counts) with and without the flag"""
    K, B, G = case["K"], case["B"], case["G"]
    mean, invstd = case["stats"][True]
    sums = torch.empty(G * 2 * C, dtype=torch.float64, device="cuda")
    count = torch.full((G,), float(B * case["H"] * case["W"]), dtype=torch.float64, device="cuda")
    K.pw_bn_backward_reduce(case["dy"], case["p"], B, mean, invstd, case["gamma"], case["beta"], sums, None, None, case["ws"])
    outs = []
    for recompute in (False, True):
        dd, dw = torch.full_like(case["p"], 7.0), torch.full((C, C, 1, 1), 7.0, device="cuda")
        K.pw_bn_backward_finish(case["dy"], case["p"], case["d"], B, mean, invstd, case["gamma"], case["beta"], case["wp"], dd, dw,
                                sums, count, case["ws"], recompute=recompute)
        outs.append((dd, dw))
    assert torch.equal(outs[1][0], outs[0][0]) and torch.equal(outs[1][1], outs[0][1])


def test_calls_the_flag_does_not_cover_read_p(case):
    """fp32 dy, or no weight gradient: the library accepts the flag and still reads p - here a p that is NOT d W^T"""
    K, B = case["K"], case["B"]
    mean, invstd = case["stats"][True]
    other_p = torch.roll(case["p"], 1, 0) if case["N"] > 1 else -case["p"]
    for dy, dweight in ((case["dy"].float(), True), (case["dy"], False)):
        res = []
        for recompute in (False, True):
            dd = torch.full_like(case["p"], 7.0)
            dw = torch.full((C, C, 1, 1), 7.0, device="cuda") if dweight else None
            K.pw_bn_backward(dy, other_p, case["d"], B, mean, invstd, case["gamma"], case["beta"], True, case["wp"], dd, None,
                             None, dw, case["ws"], recompute=recompute)
            res.append(dd)
        assert torch.equal(res[0], res[1])
