"""Kernel level of the synchronised BatchNorm (include/nvq.h, "Synchronised BatchNorm"): reduce -> finish with the local sums is
bit-identical to the one-call form, and reduce on two halves of a batch, the two sums buffers added (what the all-reduce of
two ranks does), then finish matches the one-call form over the whole batch within fp32 rounding."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
EPS, MOM = 1e-5, 0.1


@pytest.fixture(scope="module")
def K():
    from nerve_cl import _nvq
    _nvq.lib()
    return _nvq


def ws_of(K):
    from nerve_cl import _engine
    return _engine.workspace(DEV)


def rnd(*shape, seed=0, scale=1.0, offset=0.0, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(*shape, generator=g) * scale + offset).to(DEV, dtype)


def close_stats(a, b, scale_ulps=4):
    """within a few fp32 roundings of b's magnitude (the partial sums are formed over other pixel ranges)"""
    return bool((a - b).abs().max() <= scale_ulps * 1.2e-7 * b.abs().max())


def rel(a, b):
    return ((a.double() - b.double()).abs().max() / b.double().abs().max().clamp_min(1e-30)).item()


def halves(x, G, B, b0):
    """images [G * B, ...] (group-major) -> the first b0 / the other B - b0 images of every group"""
    v = x.view(G, B, *x.shape[1:])
    return v[:, :b0].reshape(G * b0, *x.shape[1:]).contiguous(), v[:, b0:].reshape(G * (B - b0), *x.shape[1:]).contiguous()


def join(a, b, G):
    return torch.cat([a.view(G, -1, *a.shape[1:]), b.view(G, -1, *b.shape[1:])], 1).reshape(-1, *a.shape[1:])


# ----------------------------------------------------------------------------- SR BatchNorm (groups of frames)
@pytest.mark.parametrize("C,dtype", [(16, torch.float32), (32, torch.float32), (64, torch.bfloat16)])
@pytest.mark.parametrize("b0", [1, 2])
def test_bn_stats_reduce_finish(K, C, dtype, b0):
    G, B, H, W = 3, 3, 12, 20
    x = rnd(G * B, H, W, C, seed=1, scale=2.0, offset=0.3, dtype=dtype)
    order = [1, 0, 2]
    ws = ws_of(K)
    rm0, rv0 = rnd(C, seed=2), rnd(C, seed=3).abs() + 0.5
    mean, invstd, rm, rv = torch.empty(G, C, device=DEV), torch.empty(G, C, device=DEV), rm0.clone(), rv0.clone()
    K.bn_stats(x, B, order, mean, invstd, rm, rv, ws, EPS, MOM)
    st = K.new_bn_stats(DEV, G, C)
    K.bn_stats_reduce(x, B, st, ws)
    m2, i2, rm2, rv2 = torch.empty_like(mean), torch.empty_like(invstd), rm0.clone(), rv0.clone()
    K.bn_stats_finish(st, G, order, m2, i2, rm2, rv2, EPS, MOM)
    for a, b in ((m2, mean), (i2, invstd), (rm2, rm), (rv2, rv)):
        assert torch.equal(a, b)
    assert torch.equal(K.bn_counts(st, G, C).cpu(), torch.full((G,), float(B * H * W), dtype=torch.float64))
    # two "ranks": the halves' sums added, then finish
    x0, x1 = halves(x, G, B, b0)
    s0, s1 = K.new_bn_stats(DEV, G, C), K.new_bn_stats(DEV, G, C)
    K.bn_stats_reduce(x0, b0, s0, ws)
    K.bn_stats_reduce(x1, B - b0, s1, ws)
    m3, i3, rm3, rv3 = torch.empty_like(mean), torch.empty_like(invstd), rm0.clone(), rv0.clone()
    K.bn_stats_finish(s0 + s1, G, order, m3, i3, rm3, rv3, EPS, MOM)
    assert close_stats(m3, mean) and close_stats(i3, invstd) and close_stats(rm3, rm) and close_stats(rv3, rv)


@pytest.mark.parametrize("b0", [1, 2])
def test_dwpw_forward_sums(K, b0):
    G, B, H, W, C = 3, 3, 12, 20, 64
    x = rnd(G * B, H, W, C, seed=4, dtype=torch.bfloat16)
    dw, pw = rnd(C, 1, 3, 3, seed=5, scale=0.3), rnd(C, C, 1, 1, seed=6, scale=0.15)
    order = [1, 0, 2]
    ws = ws_of(K)
    rm0, rv0 = rnd(C, seed=2), rnd(C, seed=3).abs() + 0.5
    d, p = torch.empty_like(x), torch.empty_like(x)
    mean, invstd, rm, rv = torch.empty(G, C, device=DEV), torch.empty(G, C, device=DEV), rm0.clone(), rv0.clone()
    K.dwpw_forward(x, None, dw, pw, d, p, B, order, mean, invstd, rm, rv, ws, EPS, MOM)
    d2, p2 = torch.empty_like(x), torch.empty_like(x)
    st = K.new_bn_stats(DEV, G, C)
    K.dwpw_forward_sums(x, None, dw, pw, d2, p2, B, st, ws)
    m2, i2, rm2, rv2 = torch.empty_like(mean), torch.empty_like(invstd), rm0.clone(), rv0.clone()
    K.bn_stats_finish(st, G, order, m2, i2, rm2, rv2, EPS, MOM)
    for a, b in ((d2, d), (p2, p), (m2, mean), (i2, invstd), (rm2, rm), (rv2, rv)):
        assert torch.equal(a, b)
    x0, x1 = halves(x, G, B, b0)
    s0, s1 = K.new_bn_stats(DEV, G, C), K.new_bn_stats(DEV, G, C)
    K.dwpw_forward_sums(x0, None, dw, pw, torch.empty_like(x0), torch.empty_like(x0), b0, s0, ws)
    K.dwpw_forward_sums(x1, None, dw, pw, torch.empty_like(x1), torch.empty_like(x1), B - b0, s1, ws)
    m3, i3, rm3, rv3 = torch.empty_like(mean), torch.empty_like(invstd), rm0.clone(), rv0.clone()
    K.bn_stats_finish(s0 + s1, G, order, m3, i3, rm3, rv3, EPS, MOM)
    assert close_stats(m3, mean) and close_stats(i3, invstd) and close_stats(rm3, rm) and close_stats(rv3, rv)


def _sr_bwd_inputs(K, G, B, H, W, C, dtype, seed):
    x = rnd(G * B, H, W, C, seed=seed, scale=1.5, offset=0.2, dtype=dtype)
    dy = rnd(G * B, H, W, C, seed=seed + 1, dtype=dtype)
    gamma, beta = rnd(C, seed=seed + 2, scale=0.5, offset=1.0), rnd(C, seed=seed + 3, scale=0.3)
    mean, invstd = torch.empty(G, C, device=DEV), torch.empty(G, C, device=DEV)
    K.bn_stats(x, B, list(range(G)), mean, invstd, None, None, ws_of(K), EPS, MOM)
    return x, dy, gamma, beta, mean, invstd


@pytest.mark.parametrize("C,dtype", [(16, torch.float32), (64, torch.bfloat16)])
@pytest.mark.parametrize("b0", [1, 2])
def test_bn_relu_backward_reduce_finish(K, C, dtype, b0):
    G, B, H, W = 3, 3, 10, 14
    x, dy, gamma, beta, mean, invstd = _sr_bwd_inputs(K, G, B, H, W, C, dtype, 10)
    ws = ws_of(K)
    dx, dg, db = torch.empty_like(x), torch.empty(C, device=DEV), torch.empty(C, device=DEV)
    K.bn_relu_backward(dy, x, B, mean, invstd, gamma, beta, True, dx, dg, db, ws)
    sums = torch.empty(G * 2 * C, dtype=torch.float64, device=DEV)
    count = torch.full((G,), float(B * H * W), dtype=torch.float64, device=DEV)
    dx2, dg2, db2 = torch.empty_like(x), torch.empty(C, device=DEV), torch.empty(C, device=DEV)
    K.bn_relu_backward_reduce(dy, x, B, mean, invstd, gamma, beta, sums, dg2, db2, ws)
    K.bn_relu_backward_finish(dy, x, B, mean, invstd, gamma, beta, sums, count, dx2)
    for a, b in ((dx2, dx), (dg2, dg), (db2, db)):
        assert torch.equal(a, b)
    (x0, x1), (d0, d1) = halves(x, G, B, b0), halves(dy, G, B, b0)
    s0, s1 = torch.empty_like(sums), torch.empty_like(sums)
    g0, g1 = torch.empty(C, device=DEV), torch.empty(C, device=DEV)
    K.bn_relu_backward_reduce(d0, x0, b0, mean, invstd, gamma, beta, s0, g0, None, ws)
    K.bn_relu_backward_reduce(d1, x1, B - b0, mean, invstd, gamma, beta, s1, g1, None, ws)
    tot = s0 + s1
    o0, o1 = torch.empty_like(x0), torch.empty_like(x1)
    K.bn_relu_backward_finish(d0, x0, b0, mean, invstd, gamma, beta, tot, count, o0)
    K.bn_relu_backward_finish(d1, x1, B - b0, mean, invstd, gamma, beta, tot, count, o1)
    assert rel(join(o0, o1, G), dx) <= (1e-5 if dtype == torch.float32 else 8e-3)
    assert rel(g0 + g1, dg) <= 1e-5


@pytest.mark.parametrize("dy_dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("b0", [1, 2])
def test_pw_bn_backward_reduce_finish(K, dy_dtype, b0):
    G, B, H, W, C = 3, 3, 10, 14, 64
    p, dy, gamma, beta, mean, invstd = _sr_bwd_inputs(K, G, B, H, W, C, torch.bfloat16, 20)
    dy = dy.to(dy_dtype)
    d = rnd(G * B, H, W, C, seed=30, dtype=torch.bfloat16)
    w = rnd(C, C, 1, 1, seed=31, scale=0.15)
    ws = ws_of(K)
    dd, dg, db, dw = torch.empty_like(p), torch.empty(C, device=DEV), torch.empty(C, device=DEV), torch.empty_like(w)
    K.pw_bn_backward(dy, p, d, B, mean, invstd, gamma, beta, True, w, dd, dg, db, dw, ws)
    sums = torch.empty(G * 2 * C, dtype=torch.float64, device=DEV)
    count = torch.full((G,), float(B * H * W), dtype=torch.float64, device=DEV)
    dd2, dg2, db2, dw2 = torch.empty_like(p), torch.empty(C, device=DEV), torch.empty(C, device=DEV), torch.empty_like(w)
    K.pw_bn_backward_reduce(dy, p, B, mean, invstd, gamma, beta, sums, dg2, db2, ws)
    K.pw_bn_backward_finish(dy, p, d, B, mean, invstd, gamma, beta, w, dd2, dw2, sums, count, ws)
    for a, b in ((dd2, dd), (dg2, dg), (db2, db), (dw2, dw)):
        assert torch.equal(a, b)
    (p0, p1), (y0, y1), (e0, e1) = halves(p, G, B, b0), halves(dy, G, B, b0), halves(d, G, B, b0)
    s0, s1 = torch.empty_like(sums), torch.empty_like(sums)
    K.pw_bn_backward_reduce(y0, p0, b0, mean, invstd, gamma, beta, s0, None, None, ws)
    K.pw_bn_backward_reduce(y1, p1, B - b0, mean, invstd, gamma, beta, s1, None, None, ws)
    tot = s0 + s1
    o0, o1, w0, w1 = torch.empty_like(p0), torch.empty_like(p1), torch.empty_like(w), torch.empty_like(w)
    K.pw_bn_backward_finish(y0, p0, e0, b0, mean, invstd, gamma, beta, w, o0, w0, tot, count, ws)
    K.pw_bn_backward_finish(y1, p1, e1, B - b0, mean, invstd, gamma, beta, w, o1, w1, tot, count, ws)
    assert rel(join(o0, o1, G), dd) <= 8e-3          # dd is stored as bf16
    assert rel(w0 + w1, dw) <= 1e-4


# ----------------------------------------------------------------------------- FrameRecoveryNet / layer BatchNorm (nvq_bn2_*)
def _bn2_stats(K, x, C, rm, rv):
    from nerve_cl._nvq import check, lib, ptr, stream
    N, H, W, ld = x.shape
    ws = ws_of(K)
    mean, invstd = torch.empty(C, device=DEV), torch.empty(C, device=DEV)
    check(lib().nvq_bn2_stats(ptr(x), ld, C, N * H * W, EPS, MOM, ptr(mean), ptr(invstd), ptr(rm), ptr(rv), ptr(ws),
                              ws.numel() * 4, int(x.dtype == torch.bfloat16), stream()), "nvq_bn2_stats")
    return mean, invstd


def _bn2_reduce(K, x, C):
    from nerve_cl._nvq import check, lib, ptr, stream
    N, H, W, ld = x.shape
    ws = ws_of(K)
    st = torch.empty(2 * C + 1, dtype=torch.float64, device=DEV)
    check(lib().nvq_bn2_stats_reduce(ptr(x), ld, C, N * H * W, ptr(st), ptr(ws), ws.numel() * 4, int(x.dtype == torch.bfloat16),
                                     stream()), "nvq_bn2_stats_reduce")
    return st


def _bn2_finish(K, st, C, rm, rv):
    from nerve_cl._nvq import check, lib, ptr, stream
    mean, invstd = torch.empty(C, device=DEV), torch.empty(C, device=DEV)
    check(lib().nvq_bn2_stats_finish(ptr(st), C, EPS, MOM, ptr(mean), ptr(invstd), ptr(rm), ptr(rv), stream()),
          "nvq_bn2_stats_finish")
    return mean, invstd


@pytest.mark.parametrize("C,ld,dtype", [(13, 16, torch.float32), (64, 64, torch.float32), (24, 24, torch.bfloat16)])
@pytest.mark.parametrize("n0", [1, 2])
def test_bn2_stats_reduce_finish(K, C, ld, dtype, n0):
    N, H, W = 3, 9, 11
    x = rnd(N, H, W, ld, seed=40, scale=2.0, offset=0.3, dtype=dtype)
    x[..., C:] = 0
    rm0, rv0 = rnd(C, seed=41), rnd(C, seed=42).abs() + 0.5
    rm, rv = rm0.clone(), rv0.clone()
    mean, invstd = _bn2_stats(K, x, C, rm, rv)
    rm2, rv2 = rm0.clone(), rv0.clone()
    st = _bn2_reduce(K, x, C)
    m2, i2 = _bn2_finish(K, st, C, rm2, rv2)
    for a, b in ((m2, mean), (i2, invstd), (rm2, rm), (rv2, rv)):
        assert torch.equal(a, b)
    assert st[2 * C].item() == N * H * W
    rm3, rv3 = rm0.clone(), rv0.clone()
    m3, i3 = _bn2_finish(K, _bn2_reduce(K, x[:n0].contiguous(), C) + _bn2_reduce(K, x[n0:].contiguous(), C), C, rm3, rv3)
    assert close_stats(m3, mean) and close_stats(i3, invstd) and close_stats(rm3, rm) and close_stats(rv3, rv)


@pytest.mark.parametrize("with_res", [False, True])
@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("C,ld,dtype", [(13, 16, torch.float32), (24, 24, torch.bfloat16)])
def test_bn2_backward_reduce_finish(K, with_res, relu, C, ld, dtype):
    from nerve_cl._nvq import check, lib, ptr, stream
    N, H, W = 3, 9, 11
    bf = int(dtype == torch.bfloat16)
    x = rnd(N, H, W, ld, seed=50, scale=1.5, offset=0.2, dtype=dtype)
    dy = rnd(N, H, W, ld, seed=51, dtype=dtype)
    res = rnd(N, H, W, ld, seed=52, scale=0.5, dtype=dtype) if with_res else None
    for t in (x, dy) + ((res,) if with_res else ()):
        t[..., C:] = 0
    gamma, beta = rnd(C, seed=53, scale=0.5, offset=1.0), rnd(C, seed=54, scale=0.3)
    mean, invstd = _bn2_stats(K, x, C, None, None)
    ws = ws_of(K)

    def one_call(dy_, x_, res_):
        n = x_.shape[0] * H * W
        dx = torch.empty_like(x_)
        dres = torch.empty_like(res_) if res_ is not None else None
        dg, db = torch.empty(C, device=DEV), torch.empty(C, device=DEV)
        check(lib().nvq_bn2_backward(ptr(dy_), ld, ptr(x_), ld, C, n, ptr(mean), ptr(invstd), ptr(gamma), ptr(beta), ptr(res_),
                                     ld if res_ is not None else 0, int(relu), 1, ptr(dx), ld, ptr(dres),
                                     ld if dres is not None else 0, ptr(dg), ptr(db), ptr(ws), ws.numel() * 4, bf, stream()),
              "nvq_bn2_backward")
        return dx, dres, dg, db

    def reduce(dy_, x_, res_):
        n = x_.shape[0] * H * W
        dres = torch.empty_like(res_) if res_ is not None else None
        dg, db = torch.empty(C, device=DEV), torch.empty(C, device=DEV)
        sums = torch.empty(2 * C, dtype=torch.float64, device=DEV)
        check(lib().nvq_bn2_backward_reduce(ptr(dy_), ld, ptr(x_), ld, C, n, ptr(mean), ptr(invstd), ptr(gamma), ptr(beta),
                                            ptr(res_), ld if res_ is not None else 0, int(relu), ptr(dres),
                                            ld if dres is not None else 0, ptr(sums), ptr(dg), ptr(db), ptr(ws), ws.numel() * 4,
                                            bf, stream()), "nvq_bn2_backward_reduce")
        return sums, dres, dg, db

    def finish(dy_, x_, dres, sums, count):
        dx = torch.empty_like(x_)
        check(lib().nvq_bn2_backward_finish(ptr(dy_), ld, ptr(x_), ld, C, x_.shape[0] * H * W, ptr(mean), ptr(invstd),
                                            ptr(gamma), ptr(beta), ptr(dres), ld if dres is not None else 0, int(relu),
                                            ptr(sums), ptr(count), ptr(dx), ld, bf, stream()), "nvq_bn2_backward_finish")
        return dx

    dx, dres, dg, db = one_call(dy, x, res)
    count = torch.tensor([float(N * H * W)], dtype=torch.float64, device=DEV)
    sums, dres2, dg2, db2 = reduce(dy, x, res)
    dx2 = finish(dy, x, dres2, sums, count)
    assert torch.equal(dx2, dx) and torch.equal(dg2, dg) and torch.equal(db2, db)
    if with_res:
        assert torch.equal(dres2, dres)
    # two ranks with 1 and 2 images
    parts = [(dy[a:b].contiguous(), x[a:b].contiguous(), res[a:b].contiguous() if with_res else None) for a, b in ((0, 1), (1, N))]
    red = [reduce(*pt) for pt in parts]
    tot = red[0][0] + red[1][0]
    dxs = [finish(pt[0], pt[1], r[1], tot, count) for pt, r in zip(parts, red)]
    assert rel(torch.cat(dxs), dx) <= (1e-5 if dtype == torch.float32 else 8e-3)
    assert rel(red[0][2] + red[1][2], dg) <= 1e-5 and rel(red[0][3] + red[1][3], db) <= 1e-5
