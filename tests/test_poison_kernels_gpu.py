"""GPU: single launches on poisoned memory (tests/_poison.py; the helper is proved by tests/test_poison_cpu.py).

Every check is a PAIR of calls on the same data: a clean one (workspace, overwritten destinations, neighbouring channels,
the other images all zero) and a poisoned one (the same places quiet NaN).  Whatever the op is documented to write must have
the same BITS in both, and the clean result must meet the float64 / PyTorch reference bound of the neighbouring test in
tests/test_kernels_gpu.py (named at each check), so that a pair of identically wrong results does not pass.  Bytes of a
destination tensor outside the written slice must still be NaN (zero in the clean call) afterwards.

  (a) workspace and destination: every op that takes a `ws`, every op with an overwrite mode
  (b) neighbour slices: the `Sl` input at a non-zero channel offset in a wider tensor whose other channels are NaN; channels
      that a contract requires to be zero (the padding up to the stored width: pad4, cin_store) stay zero, the poison begins
      behind them
  (c) images are independent: image 1 of 3 all NaN, images 0 and 2 of the output untouched by it
  (d) one bad pixel stays local: a NaN at one pixel (every channel) reaches the 3x3 neighbourhood of a 3x3 conv and that
      pixel of a 1x1 conv, and nothing else

Integer and index buffers (one-bit ReLU masks, the CBAM arg-max plane, the warp gather's hit lists) are never poisoned, and
the warp's flow field - a float tensor used as a coordinate - is never a poisoned input: tests/_poison.py says why.  No
tolerance here is measured: every bound is exact equality or an existing bound of the neighbouring test."""
import time

import pytest
import torch
import torch.nn.functional as F

import _poison as P
import test_launch_forms_cpu as LF
from oracle import sr_oracle
from test_kernels_gpu import TOL, bf, from_nhwc, rel, rnd, to_nhwc

pytestmark = pytest.mark.gpu

BF16_ONE_ROUNDING = 5e-3        # "one bf16 rounding of the result" (tests/test_kernels_gpu.py, tests/_sr_replay.py TOL_BF16)
GRAD_TOL = 5e-5                 # fp32 gradients with a longer reduction (test_batchnorm_relu_groups, test_cbam_forward_backward)
B16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
N2, H, W = 2, 17, 35            # 3 x 2 tiles of 8 x 32 per image, ragged in both directions
PIXELS = [(0, 0), (7, 31), (8, 32), (H - 1, W - 1)]       # the image corners and both sides of a tile seam
HB, WB = 37, 41                 # 1517 pixels: two blocks of the 1024-pixel pooling reductions (nvq_tsum_blocks), the second ragged


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device")
    from nerve_cl import _nvq
    _nvq.lib()
    t0 = time.perf_counter()
    yield _nvq
    print(f"\nPOISON-FILE tests/test_poison_kernels_gpu.py wall {time.perf_counter() - t0:.1f} s")


@pytest.fixture(scope="module")
def consts():
    return LF.host_constants()


_WS = {}


def _workspace(K, slot=0):
    if slot not in _WS:
        _WS[slot] = torch.empty(K.wgrad_workspace_bytes() // 4 + (1 << 20), dtype=F32, device="cuda")
    return _WS[slot]


class Mem:
    """the memory of one call of a pair: `poison` decides whether the places nobody may read hold NaN or zeros"""

    def __init__(self, K, poison):
        self.K, self.poison, self.bytes = K, poison, 0

    def fill(self, t):
        if self.poison:
            P.poison_(t)
            self.bytes += t.numel() * t.element_size()
        else:
            t.zero_()
        return t

    def dest(self, *shape, dtype=F32):
        """an overwritten destination"""
        return self.fill(torch.empty(*shape, dtype=dtype, device="cuda"))

    def ws(self, slot=0):
        return self.fill(_workspace(self.K, slot))

    def wide(self, x, ld, coff, zero_to=None, dtype=F32):
        """CPU NCHW -> cuda [N,H,W,ld] with x at channels [coff, coff + C), zeros up to `zero_to` (a contract's padding),
        NaN / zeros everywhere else"""
        n, c, h, w = x.shape
        buf = self.dest(n, h, w, ld, dtype=dtype)
        buf[..., coff:coff + c] = x.permute(0, 2, 3, 1).to(dtype).cuda()
        end = coff + c
        if zero_to is not None and zero_to > end:
            buf[..., end:zero_to] = 0
            end = zero_to
        if self.poison:
            self.bytes -= n * h * w * (end - coff) * buf.element_size()
        return buf


def pair(name, form, fn, verify, K):
    """fn(mem) -> {key: tensor}; keys starting with 'untouched:' are the parts of a destination tensor outside the written
    slice.  verify(outs) asserts the neighbouring test's reference bound on the clean outputs."""
    clean = fn(Mem(K, False))
    mem = Mem(K, True)
    poisoned = fn(mem)
    torch.cuda.synchronize()
    assert sorted(clean) == sorted(poisoned) and mem.bytes > 0
    print(f"\nPOISON kernel {name:44s} form {form:40s} bytes {mem.bytes:10d}", end=" ")
    for k in clean:
        if k.startswith("untouched:"):
            assert not clean[k].float().any(), f"{name}: {k} was written (clean call)"
            assert bool(torch.isnan(poisoned[k].float()).all()), f"{name}: {k} was written (poisoned call)"
        else:
            assert bool(torch.isfinite(clean[k].double()).all()), f"{name}: {k} is not finite on clean memory"
            P.assert_same_bits(clean[k], poisoned[k], f"{name}: {k}, clean against poisoned")
    verify(clean)
    print("pass")


def nchw(t, c=None, coff=0):
    return from_nhwc(t.float(), c, coff)


def planar_input(K, m, xv, cin, planar_F):
    """xv (CPU NCHW, bf16-representable) as a slice-planar CatBuf with one more plane than `cin` reads; that plane and
    anything else of the allocation that holds no data is the Mem's filler"""
    n, _, h, w = xv.shape
    cat = K.CatBuf("cuda", n, h, w, planar_F, (cin - planar_F) // 32 + 1, 256, B16, planar=True)
    m.fill(cat.flat)
    xn = to_nhwc(xv).bfloat16()
    cat.lead.copy_(xn[..., :planar_F])
    for j in range((cin - planar_F) // 32):
        cat.slices[j].copy_(xn[..., planar_F + 32 * j:planar_F + 32 * (j + 1)])
    if m.poison:
        m.bytes -= xn.numel() * 2
    return cat.inp(cin)               # (a view of cat.flat: the allocation lives as long as the slice)


def images_and_bad_pixels(K, name, run, x, k):
    """(c) and (d) for run(mem, values) -> [3, H, W, C] on the values x [3, C', H, W]: image 1 all NaN leaves images 0 and 2 with the
    bits of the clean call; one NaN pixel (every channel) of image 0, at each of PIXELS, turns every channel of the k x k
    neighbourhood NaN and leaves every other element with the bits of the clean call.  -> the clean result"""
    clean = run(Mem(K, False), x)
    xv = x.clone()
    xv[1] = float("nan")
    got = run(Mem(K, True), xv)
    P.assert_same_bits(clean[0], got[0], f"{name}: image 0 beside a NaN image")
    P.assert_same_bits(clean[2], got[2], f"{name}: image 2 beside a NaN image")
    assert bool(torch.isnan(got[1].float()).all())
    r = k // 2
    for (py, px) in PIXELS:
        xv = x.clone()
        xv[0, :, py, px] = float("nan")
        got = run(Mem(K, True), xv)
        hit = torch.zeros(got.shape[:3], dtype=torch.bool, device="cuda")
        hit[0, max(0, py - r):py + r + 1, max(0, px - r):px + r + 1] = True
        isn = torch.isnan(got.float())
        assert torch.equal(isn.all(-1), hit) and torch.equal(isn.any(-1), hit), f"{name}: NaN pixel ({py},{px}) spread"
        keep = ~hit[..., None].expand_as(got)
        P.assert_same_bits(clean[keep], got[keep], f"{name}: pixels away from the NaN at ({py},{px})")
    return clean


def test_the_pair_is_live_on_the_two_defects_it_is_meant_for(K):
    """seeded on the GPU, with the library's own kernels called against their contract: (1) an epilogue that READS its
    destination (accumulate = True into a destination that the pair treats as overwritten); (2) an over-read that is masked by
    a multiplication - the slice handed to the conv is 8 channels wider than the data and only the zero weights of those 8
    channels keep the neighbour out, which passes every value check on clean memory.  Both must be flagged, and the same calls
    within the contract must pass."""
    x, wt = rnd(N2, 40, H, W), rnd(32, 40, 3, 3, scale=0.2)
    want = F.conv2d(x, wt, None, padding=1)
    wz = torch.cat([wt, torch.zeros(32, 8, 3, 3)], 1)
    wp40, wp48 = K.conv_pack(wt.cuda(), False, 40), K.conv_pack(wz.cuda(), False, 48)

    def call(accumulate, over_read):
        def fn(m):
            xt = m.wide(x, 64, 8)
            out = m.dest(N2, H, W, 32)
            K.conv_forward(K.Sl(xt, 48 if over_read else 40, 8), wp48 if over_read else wp40, None, K.Sl(out), 3, accumulate=accumulate)
            return {"y": out}
        return fn

    def verify(o):
        assert rel(nchw(o["y"]), want) < TOL

    pair("seeded: within the contract", "conv_f32_kernel", call(False, False), verify, K)
    with pytest.raises(AssertionError, match="clean against poisoned"):
        pair("seeded: epilogue reads its destination", "conv_f32_kernel, accumulate", call(True, False), verify, K)
    with pytest.raises(AssertionError, match="clean against poisoned"):
        pair("seeded: neighbour times zero weight", "conv_f32_kernel, 48-channel slice", call(False, True), verify, K)
    print("(both seeded defects flagged)")


# =============================================================================== (a) workspace and destination
def _conv_ref_grads(x, dy, cout, cin, k, alpha=1.0):
    w = torch.zeros(cout, cin, k, k, requires_grad=True)
    (F.conv2d(x, w, None, padding=k // 2) * alpha).backward(dy)
    return w.grad, alpha * dy.sum((0, 2, 3))


WGRAD_CASES = {
    # name: (cin, cin_store, cout, k, math, x bf16, dy bf16, planar F, variant, alpha, form)
    "wgrad f32 64->32 k3": (64, 64, 32, 3, "f32", False, False, 0, 0, 1.0, None),
    "wgrad f32 81(96)->128 k3": (81, 96, 128, 3, "f32", False, False, 0, 0, 0.5, None),
    "wgrad f32 224->64 k1": (224, 224, 64, 1, "f32", False, False, 0, 0, 1.0, None),
    "wgrad f32 64->12 k3": (64, 64, 12, 3, "f32", False, False, 0, 0, 1.0, None),
    "wgrad bf16-math fp32-stored 64->32 k3": (64, 64, 32, 3, "bf16", False, False, 0, 0, 1.0, "wgrad_bf16_kernel<3,f,f,32>"),
    "wgrad bf16-math fp32-stored 81(96)->128 k3": (81, 96, 128, 3, "bf16", False, False, 0, 0, 1.0, "wgrad_bf16_kernel<3,f,f,32>"),
    "wgrad bf16 x, fp32 dy 64->32 k3": (64, 64, 32, 3, "bf16", True, False, 0, 0, 1.0, "wgrad_bf16_kernel<3,t,f,32>"),
    "wgrad fp32 x, bf16 dy 64->32 k3": (64, 64, 32, 3, "bf16", False, True, 0, 0, 1.0, "wgrad_bf16_kernel<3,f,t,32>"),
    "wgrad bf16 32->32 k3": (32, 32, 32, 3, "bf16", True, True, 0, 0, 1.0, "wgrad_bf16_kernel<3,t,t,32> (32-ci workgroups)"),
    "wgrad bf16 64->32 k3": (64, 64, 32, 3, "bf16", True, True, 0, 0, 1.0, "wgrad_bf16_kernel<3,t,t,64> (64-ci workgroups)"),
    "wgrad bf16 96->32 k3 interleaved": (96, 96, 32, 3, "bf16", True, True, 0, 0, 0.2, "wgrad_bf16_mixed_kernel (64 + 32 ci)"),
    "wgrad bf16 192->64 k3": (192, 192, 64, 3, "bf16", True, True, 0, 0, 1.0, "wgrad_bf16_kernel<3,t,t,64,64,8> (64 co)"),
    "wgrad bf16 96->128 k3": (96, 96, 128, 3, "bf16", True, True, 0, 0, 1.0, "wgrad_bf16_kernel<3,t,t,64,64,8> (64 co)"),
    "wgrad bf16 192->64 k3 variant 3": (192, 192, 64, 3, "bf16", True, True, 0, 3, 1.0, "wgrad_bf16_kernel<3,t,t,64> (32 co)"),
    "wgrad bf16 224->64 k1": (224, 224, 64, 1, "bf16", True, True, 0, 1, 1.0, "wgrad_bf16_kernel<1,t,t,64,64> (64 co)"),
    "wgrad bf16 64->32 k1": (64, 64, 32, 1, "bf16", True, True, 0, 1, 1.0, "wgrad_bf16_kernel<1,t,t,64>"),
    "wgrad bf16 planar 96->32 k3 split": (96, 96, 32, 3, "bf16", True, True, 64, 1, 1.0, "split kernel on a slice-planar x"),
    "wgrad_m32 planar 3 blocks": (96, 96, 32, 3, "bf16", True, True, 64, 2, 1.0, "wgrad_m32_kernel<3>"),
    "wgrad_m32 planar 4 blocks": (128, 128, 32, 3, "bf16", True, True, 64, 2, 0.5, "wgrad_m32_kernel<4>"),
    "wgrad_m32 planar 5 blocks": (160, 160, 32, 3, "bf16", True, True, 64, 2, 1.0, "wgrad_m32_kernel<5>"),
    "wgrad_m32 planar 6 blocks": (192, 192, 32, 3, "bf16", True, True, 64, 2, 1.0, "wgrad_m32_kernel<6>"),
    "wgrad_m32 planar 5 blocks, F 32": (160, 160, 32, 3, "bf16", True, True, 32, 2, 1.0, "wgrad_m32_kernel<5>, lead 32"),
    "wgrad1_m32 128->32 k1": (128, 128, 32, 1, "bf16", True, True, 0, 2, 1.0, "wgrad1_m32_kernel<4,1>"),
    "wgrad1_m32 256->64 k1": (256, 256, 64, 1, "bf16", True, True, 0, 2, 1.0, "wgrad1_m32_kernel<8,2>"),
    "wgrad1_m32 planar 224->64 k1": (224, 224, 64, 1, "bf16", True, True, 64, 2, 0.2, "wgrad1_m32_kernel<7,2>, slice-planar"),
}


def _wgrad_operands(K, m, x, dy, cin, cs, cout, xb, yb, planar_F):
    """x as a slice at channel 8 of a wider tensor (or a slice-planar buffer with one more plane than is read), dy likewise;
    the cin_store / pad4 padding is zero, everything beyond is the Mem's filler"""
    if planar_F:
        xs = planar_input(K, m, x, cin, planar_F)
    else:
        xt = m.wide(x, 8 + cs + 8, 8, zero_to=8 + cs, dtype=B16 if xb else F32)
        xs = K.Sl(xt, cs, 8)
    pad = 8 if yb else 4
    cp = (cout + pad - 1) // pad * pad
    dt = m.wide(dy, 8 + cp + 8, 8, zero_to=8 + cp, dtype=B16 if yb else F32)
    return xs, K.Sl(dt, cout, 8)


@pytest.mark.parametrize("name", list(WGRAD_CASES))
def test_conv_wgrad_workspace_destination_and_neighbours(K, consts, name):
    """nvq_conv_wgrad, overwrite mode: the workspace, dw and dbias, the channels beside the x and dy slices.  Bound: TOL of
    test_conv_weight_gradient / test_conv_bf16_stored_weight_gradient / ..._all_input_channels (autograd of F.conv2d on the
    same values; the bias gradient is the plain sum of dy)."""
    cin, cs, cout, k, math, xb, yb, planar_F, variant, alpha, form = WGRAD_CASES[name]
    x, dy = rnd(N2, cin, H, W), rnd(N2, cout, H, W, seed=3)
    if math == "bf16":
        x, dy = bf(x), bf(dy)
        # variant 2 is refused by the library for a shape that the all-input-channel kernel does not take; the other bf16 forms
        # are what csrc/conv_bf16.hip's conv_wgrad_bf16 is read to choose for these channel counts and storage types - the
        # intended form, which no rule mirror recomputes
        form = ("forced by variant 2: " if variant == 2 else "intended: ") + form
    else:
        r = LF.wgrad_f32_rule(consts, cin, cout, N2, H, W)
        form = f"wgrad_f32_kernel<{k}> nsplit {r['nsplit']} tiles {r['tiles']}"
        assert r["ntiles"] > 1
    dw_ref, db_ref = _conv_ref_grads(x, dy, cout, cin, k, alpha)

    def fn(m):
        xs, ds = _wgrad_operands(K, m, x, dy, cin, cs, cout, xb, yb, planar_F)
        dw, db = m.dest(cout, cin, k, k), m.dest(cout)
        K.conv_wgrad(xs, cin, ds, dw, db, m.ws(), k, alpha=alpha, math=K.MATH_BF16 if math == "bf16" else K.MATH_F32,
                     variant=variant)
        return {"dw": dw, "dbias": db}

    def verify(o):
        assert rel(o["dw"], dw_ref) < TOL and rel(o["dbias"], db_ref) < TOL

    pair(name, form, fn, verify, K)


def test_conv_wgrad_deferred_reduce_batch(K):
    """nvq_conv_wgrad_partial x 3 into workspaces of their own, then one nvq_wgrad_reduce_batch: as
    test_conv_wgrad_in_two_halves_with_batched_reduces, bound TOL against autograd"""
    shapes = [(64, 32, 3), (96, 72, 1), (192, 32, 3)]
    data = []
    for i, (cin, cout, k) in enumerate(shapes):
        x, dy = bf(rnd(N2, cin, H, W, seed=i)), bf(rnd(N2, cout, H, W, seed=100 + i))
        data.append((cin, cout, k, x, dy, _conv_ref_grads(x, dy, cout, cin, k)))

    def fn(m):
        jobs, outs = [], {}
        for i, (cin, cout, k, x, dy, _) in enumerate(data):
            xs, ds = _wgrad_operands(K, m, x, dy, cin, cin, cout, True, True, 0)
            dw, db = m.dest(cout, cin, k, k), m.dest(cout)
            K.conv_wgrad(xs, cin, ds, dw, db, m.ws(i), k, math=K.MATH_BF16, defer=jobs)
            outs[f"dw{i}"], outs[f"dbias{i}"] = dw, db
        K.wgrad_reduce_batch(jobs)
        return outs

    def verify(o):
        for i, (*_, (dw_ref, db_ref)) in enumerate(data):
            assert rel(o[f"dw{i}"], dw_ref) < TOL and rel(o[f"dbias{i}"], db_ref) < TOL

    pair("conv_wgrad deferred + wgrad_reduce_batch", "3 partial launches, one batched reduce", fn, verify, K)


def test_head_forward_and_wgrad(K):
    """bound: TOL of test_head_forward_and_wgrad"""
    Fc, B, T = 32, 2, 3
    frames = rnd(B, T, 3, H, W).abs()
    w = rnd(Fc, 3, 3, 3, scale=0.4).requires_grad_()
    b = rnd(Fc, scale=0.1).requires_grad_()
    slots = [1, 0, 2]
    ref = torch.stack([F.relu(F.conv2d(frames[:, t], w, b, padding=1)) for t in slots], 0)
    dout = rnd(T, B, Fc, H, W, seed=4)
    ref.backward(dout)

    def fn(m):
        out = m.dest(T * B, H, W, Fc)
        K.head_forward(frames.cuda(), slots, w.detach().cuda(), b.detach().cuda(), out)
        dw, db = m.dest(Fc, 3, 3, 3), m.dest(Fc)
        K.head_wgrad(frames.cuda(), slots, to_nhwc(dout.reshape(T * B, Fc, H, W)), out, dw, db, m.ws())
        return {"out": out, "dw": dw, "dbias": db}

    def verify(o):
        assert rel(nchw(o["out"]), ref.detach().reshape(T * B, Fc, H, W)) < TOL
        assert rel(o["dw"], w.grad) < TOL and rel(o["dbias"], b.grad) < TOL

    pair("head_forward + head_wgrad", "head_wgrad_kernel<3>", fn, verify, K)


@pytest.mark.parametrize("C,bf16", [(32, False), (16, False), (64, True)], ids=["fp32-C32", "fp32-C16", "bf16-C64"])
def test_depthwise_forward_flip_wgrad(K, consts, C, bf16):
    """bounds: TOL of test_depthwise_forward_flip_wgrad / test_dwconv_bf16_full_line_kernels (fp32 outputs)"""
    x, w, dy = rnd(N2, C, H, W), rnd(C, 1, 3, 3), rnd(N2, C, H, W, seed=6)
    if bf16:
        x, dy = bf(x), bf(dy)
    xg, wg = x.clone().requires_grad_(), w.clone().requires_grad_()
    y = F.conv2d(xg, wg, None, padding=1, groups=C)
    y.backward(dy)
    r = LF.dw_rule(consts, C, N2, H, W, bf16)
    dt = B16 if bf16 else F32

    def fn(m):
        xb, dyb = to_nhwc(x).to(dt), to_nhwc(dy).to(dt)
        out, dx, dw = m.dest(N2, H, W, C), m.dest(N2, H, W, C), m.dest(C, 1, 3, 3)
        K.dwconv_forward(xb, w.cuda(), out)
        K.dwconv_forward(dyb, w.cuda(), dx, flip=True)
        K.dwconv_wgrad(xb, dyb, dw, m.ws())
        return {"out": out, "dx": dx, "dw": dw}

    def verify(o):
        assert rel(nchw(o["out"]), y.detach()) < TOL and rel(nchw(o["dx"]), xg.grad) < TOL and rel(o["dw"], wg.grad) < TOL

    pair(f"dwconv forward / flip / wgrad C{C}", f"{r['form']} tiles {r['tiles']} wg {r['wg']}", fn, verify, K)


@pytest.mark.parametrize("with_bn", [False, True], ids=["plain", "bn-input"])
def test_dwconv_backward_from_one_tile(K, with_bn):
    """nvq_dwconv_backward: bounds of test_depthwise_backward_input_and_weight_gradient_from_one_tile (dx one bf16 rounding,
    dweight TOL)"""
    C, B, G = 64, 1, 2
    x = bf(rnd(N2, C, H, W, seed=1) * 1.5 + 0.2)
    dy = bf(rnd(N2, C, H, W, seed=2))
    wd = rnd(C, 1, 3, 3, seed=3)
    gamma, beta = (1 + 0.2 * rnd(C, seed=4)).cuda(), (0.1 * rnd(C, seed=5)).cuda()
    state = {}

    def fn(m):
        xb, dyb = to_nhwc(x).bfloat16(), to_nhwc(dy).bfloat16()
        bn = None
        if with_bn:
            m0, i0 = m.dest(G, C), m.dest(G, C)
            K.bn_stats(xb, B, list(range(G)), m0, i0, None, None, m.ws())
            bn = (m0, i0, gamma, beta, B)
            r = m.dest(N2, H, W, C, dtype=B16)
            K.bn_apply_relu(xb, B, m0, i0, gamma, beta, None, K.Sl(r), N2)
            state["xin"] = nchw(r)
        dx, dw = m.dest(N2, H, W, C, dtype=B16), m.dest(C, 1, 3, 3)
        K.dwconv_backward(xb, bn, dyb, wd.cuda(), dx, dw, m.ws())
        return {"dx": dx, "dw": dw}

    def verify(o):
        xg, wg = (state["xin"] if with_bn else x).clone().requires_grad_(), wd.clone().requires_grad_()
        F.conv2d(xg, wg, None, padding=1, groups=C).backward(dy)
        assert rel(nchw(o["dx"]), xg.grad) < BF16_ONE_ROUNDING and rel(o["dw"], wg.grad) < TOL

    pair(f"dwconv_backward {'bn input' if with_bn else 'plain'}", "dw_bwd_kernel 64 channels", fn, verify, K)


@pytest.mark.parametrize("C,bf16", [(32, False), (64, True)], ids=["fp32-C32", "bf16-C64"])
def test_batchnorm_statistics_apply_backward_and_the_reduce_finish_pair(K, C, bf16):
    """nvq_bn_stats / bn_apply_relu / bn_relu_backward and the synchronised pair (bn_stats_reduce + finish, bn_relu_backward_reduce
    + finish).  Bounds: test_batchnorm_relu_groups (TOL forward and running statistics, 5e-5 gradients),
    test_extractor_kernels_with_bf16_stored_tensors for the bf16-stored tensors (5e-3 / 8e-3); the pair equals the one-call
    form bit for bit (tests/test_sync_bn_kernels_gpu.py)."""
    B, G = 1, 2
    x = rnd(N2, C, H, W) * 1.5 + 0.3
    dy = rnd(N2, C, H, W, seed=12)
    if bf16:
        x, dy = bf(x), bf(dy)
    xg = x.clone().requires_grad_()
    gamma, beta = (1 + 0.2 * rnd(C)).requires_grad_(), (0.1 * rnd(C, seed=2)).requires_grad_()
    rm, rv = 0.1 * rnd(C, seed=3), 1 + 0.3 * rnd(C, seed=4)
    order = [1, 0]
    rm_ref, rv_ref = rm.clone(), rv.clone()
    ys = [None] * G
    for g in order:
        ys[g] = F.relu(F.batch_norm(xg[g * B:(g + 1) * B], rm_ref, rv_ref, gamma, beta, True, 0.1, 1e-5))
    y = torch.cat(ys, 0)
    y.backward(dy)
    dt = B16 if bf16 else F32
    gc, bc = gamma.detach().cuda(), beta.detach().cuda()

    def fn(m):
        xb, dyb = to_nhwc(x).to(dt), to_nhwc(dy).to(dt)
        mean, invstd, rmc, rvc = m.dest(G, C), m.dest(G, C), rm.cuda(), rv.cuda()
        K.bn_stats(xb, B, order, mean, invstd, rmc, rvc, m.ws())
        wide = m.dest(B, H, W, 3 * C, dtype=dt)
        outB = m.dest(N2 - B, H, W, C, dtype=dt)
        K.bn_apply_relu(xb, B, mean, invstd, gc, bc, None, K.Sl(wide, C, C), B, K.Sl(outB))
        dx, dg, db = m.dest(N2, H, W, C, dtype=dt), m.dest(C), m.dest(C)
        K.bn_relu_backward(dyb, xb, B, mean, invstd, gc, bc, True, dx, dg, db, m.ws())
        # the pair
        st = m.dest(G * 2 * C + G, dtype=F64)
        K.bn_stats_reduce(xb, B, st, m.ws())
        m2, i2, rm2, rv2 = m.dest(G, C), m.dest(G, C), rm.cuda(), rv.cuda()
        K.bn_stats_finish(st, G, order, m2, i2, rm2, rv2)
        sums = m.dest(G * 2 * C, dtype=F64)
        dx2, dg2, db2 = m.dest(N2, H, W, C, dtype=dt), m.dest(C), m.dest(C)
        K.bn_relu_backward_reduce(dyb, xb, B, mean, invstd, gc, bc, sums, dg2, db2, m.ws())
        K.bn_relu_backward_finish(dyb, xb, B, mean, invstd, gc, bc, sums, K.bn_counts(st, G, C), dx2)
        return {"mean": mean, "invstd": invstd, "running_mean": rmc, "running_var": rvc, "yA": wide[..., C:2 * C].contiguous(),
                "untouched:yA": torch.cat([wide[..., :C], wide[..., 2 * C:]], -1), "yB": outB, "dx": dx, "dgamma": dg, "dbeta": db,
                "mean2": m2, "invstd2": i2, "running_mean2": rm2, "running_var2": rv2, "stats": st, "sums": sums, "dx2": dx2,
                "dgamma2": dg2, "dbeta2": db2}

    def verify(o):
        assert rel(o["running_mean"], rm_ref) < TOL and rel(o["running_var"], rv_ref) < TOL
        ftol, gtol = (BF16_ONE_ROUNDING, 8e-3) if bf16 else (TOL, GRAD_TOL)
        assert rel(nchw(o["yA"]), y.detach()[:B]) < ftol and rel(nchw(o["yB"]), y.detach()[B:]) < ftol
        assert rel(nchw(o["dx"]), xg.grad) < gtol
        assert rel(o["dgamma"], gamma.grad) < GRAD_TOL and rel(o["dbeta"], beta.grad) < GRAD_TOL
        for a in ("mean", "invstd", "running_mean", "running_var", "dx", "dgamma", "dbeta"):
            assert torch.equal(o[a + "2"], o[a]), a

    pair(f"bn_stats / apply / backward / reduce+finish C{C}", "per-group statistics, 2 groups", fn, verify, K)


@pytest.mark.parametrize("recompute", [False, True], ids=["read-p", "NVQ_PW_RECOMPUTE"])
@pytest.mark.parametrize("dy16", [True, False], ids=["dy-bf16", "dy-fp32"])
def test_pw_bn_backward(K, recompute, dy16):
    """nvq_pw_bn_backward(_ex): bounds of tests/test_pw_bn_recompute_gpu.py::test_recomputed_p_gives_the_same_bits (dd 1.5e-2,
    dweight 1e-2, dgamma / dbeta 1e-4, against autograd on the stored p); d and p come from nvq_dwpw_forward on poisoned
    destinations, so that launch is part of the pair too"""
    C, B, G = 64, 1, 2
    x = (rnd(N2, H, W, C, seed=1) * 1.5 + 0.2).cuda().bfloat16()
    wd, wp = rnd(C, 1, 3, 3, seed=2).cuda(), rnd(C, C, 1, 1, seed=3, scale=0.15).cuda()
    gamma, beta = (1 + 0.2 * rnd(C, seed=4)).cuda(), (0.1 * rnd(C, seed=5)).cuda()
    rm, rv = (0.1 * rnd(C, seed=6)).cuda(), (1 + 0.3 * rnd(C, seed=7).abs()).cuda()
    dy = rnd(N2, H, W, C, seed=8).cuda().bfloat16()
    dy = dy if dy16 else dy.float()

    def fn(m):
        d, p = m.dest(N2, H, W, C, dtype=B16), m.dest(N2, H, W, C, dtype=B16)
        mean, invstd = m.dest(G, C), m.dest(G, C)
        K.dwpw_forward(x, None, wd, wp, d, p, B, list(range(G)), mean, invstd, rm.clone(), rv.clone(), m.ws())
        dd, dg, db, dw = m.dest(N2, H, W, C, dtype=B16), m.dest(C), m.dest(C), m.dest(C, C, 1, 1)
        K.pw_bn_backward(dy, p, d, B, mean, invstd, gamma, beta, True, wp, dd, dg, db, dw, m.ws(), recompute=recompute)
        return {"d": d, "p": p, "mean": mean, "invstd": invstd, "dd": dd, "dgamma": dg, "dbeta": db, "dw": dw}

    def verify(o):
        pl = nchw(o["p"]).requires_grad_()
        gg, bg = gamma.cpu().requires_grad_(), beta.cpu().requires_grad_()
        outs = [F.relu(F.batch_norm(pl[g * B:(g + 1) * B], None, None, gg, bg, True, 0.1, 1e-5)) for g in range(G)]
        torch.cat(outs, 0).backward(nchw(dy))
        dp16, w16 = bf(pl.grad), bf(wp.cpu())
        assert rel(nchw(o["dd"]), F.conv_transpose2d(dp16, w16)) < 1.5e-2
        assert rel(o["dw"].reshape(C, C), torch.einsum("nohw,nihw->oi", dp16, nchw(o["d"]))) < 1e-2
        assert rel(o["dgamma"], gg.grad) < 1e-4 and rel(o["dbeta"], bg.grad) < 1e-4
        # and d, p themselves: test_depthwise_pointwise_batchnorm_sums_forward_in_one_pass (5e-3, 8e-3)
        d_ref = F.conv2d(nchw(x), wd.cpu(), None, padding=1, groups=C)
        assert rel(nchw(o["d"]), d_ref) < 5e-3 and rel(nchw(o["p"]), F.conv2d(bf(d_ref), bf(wp.cpu()))) < 8e-3

    pair(f"dwpw_forward + pw_bn_backward {'recompute' if recompute else 'read p'} {'bf16' if dy16 else 'fp32'} dy",
         "pw_bn_bwd_kernel", fn, verify, K)


def test_colsum_and_axpy_slice(K):
    """bound: TOL of test_axpy_slice_and_colsum"""
    b = rnd(N2, 32, H, W, seed=2)

    def fn(m):
        src = m.wide(b, 96, 32)
        out = m.dest(32)
        K.colsum(K.Sl(src, 32, 32), out, m.ws(), alpha=2.0)
        dst = m.dest(N2, H, W, 64)
        K.axpy_slice(K.Sl(dst, 32, 16), K.Sl(src, 32, 32), alpha=0.5, accumulate=False)
        return {"colsum": out, "axpy": dst[..., 16:48].contiguous(), "untouched:axpy": torch.cat([dst[..., :16], dst[..., 48:]], -1)}

    def verify(o):
        assert rel(o["colsum"], 2 * b.sum((0, 2, 3))) < TOL and rel(nchw(o["axpy"]), 0.5 * b) < 1e-6

    pair("colsum + axpy_slice (overwrite)", "slice of a 96-channel tensor", fn, verify, K)


def _engine_pair(name, form, fn, verify, K, monkeypatch):
    """for the ops reached through their front ends (nerve_cl._ops / ops / metrics), which take the engine's cached workspace
    and allocate their outputs with torch.empty: clean = zeroed workspace, poisoned = NaN workspace + poisoned_allocations"""
    from nerve_cl import _engine
    dev = torch.device("cuda", torch.cuda.current_device())
    caches = lambda: list(_engine._ws_cache.values())    # noqa: E731
    _engine.workspace(dev)
    for ws in caches():
        ws.zero_()
    clean = fn()
    with monkeypatch.context() as mp:
        log = P.poisoned_allocations(mp)
        nbytes = 0
        for ws in caches():
            P.poison_(ws)
            nbytes += ws.numel() * ws.element_size()
        poisoned = fn()
        torch.cuda.synchronize()
        nbytes += log.bytes
    assert sorted(clean) == sorted(poisoned) and log.tensors > 0
    print(f"\nPOISON kernel {name:44s} form {form:40s} bytes {nbytes:10d}", end=" ")
    for k in clean:
        assert bool(torch.isfinite(clean[k].double()).all()), f"{name}: {k} is not finite on clean memory"
        P.assert_same_bits(clean[k], poisoned[k], f"{name}: {k}, clean against poisoned")
    verify(clean)
    print("pass")


@pytest.mark.parametrize("C,ld,bf16,res", [(64, 64, False, True), (13, 16, False, False), (24, 24, True, True)],
                         ids=["fp32-C64-res", "fp32-C13-in-16", "bf16-C24-res"])
def test_bn2_statistics_and_backward_of_fr_ops(K, monkeypatch, C, ld, bf16, res):
    """nvq_bn2_stats / bn2_apply / bn2_backward through nerve_cl._ops.BatchNorm on N * H * W = 1190 pixels (bn2_nblk > 1).
    The channels [C, ld) of x, dy and res are zero: tests/test_sync_bn_kernels_gpu.py::test_bn2_stats_reduce_finish sets
    `x[..., C:] = 0` for these kernels (the padding up to the stored width), and whoever owns the tensor produces those zeros -
    asserted on the op's own output below.  Bounds: tests/_sr_replay.py TOL_F32_FWD 2e-5 / TOL_F32_GRAD 2e-4 (TOL_BF16 5e-3 per
    bf16 rounding), as tests/test_fr_replay_gpu.py applies them to this op."""
    from nerve_cl import _ops
    import _sr_replay as R
    dt = B16 if bf16 else F32
    x, dy, rs = rnd(N2, C, H, W) * 1.5 + 0.3, rnd(N2, C, H, W, seed=5), rnd(N2, C, H, W, seed=6)
    if bf16:
        x, dy, rs = bf(x), bf(dy), bf(rs)
    g0, b0 = 1 + 0.2 * rnd(C), 0.1 * rnd(C, seed=2)
    xd, gd, bd = x.double().requires_grad_(), g0.double().requires_grad_(), b0.double().requires_grad_()
    rd = rs.double().requires_grad_()
    yr = F.batch_norm(xd, None, None, gd, bd, True, 0.1, 1e-5)
    yr = F.relu(yr + rd) if res else F.relu(yr)
    yr.backward(dy.double())

    def fn():
        xb = to_nhwc(x, ld).to(dt).requires_grad_()
        rb = to_nhwc(rs, ld).to(dt).requires_grad_() if res else None
        g, b = g0.cuda().requires_grad_(), b0.cuda().requires_grad_()
        rm, rv = torch.zeros(C, device="cuda"), torch.ones(C, device="cuda")
        y = _ops.BatchNorm.apply(xb, g, b, rb, rm, rv, True, True)
        y.backward(to_nhwc(dy, ld).to(dt))
        out = {"y": y.detach(), "dx": xb.grad, "dgamma": g.grad, "dbeta": b.grad, "running_mean": rm, "running_var": rv}
        if res:
            out["dres"] = rb.grad
        return out

    def verify(o):
        ftol, gtol = (R.TOL_BF16, 2 * R.TOL_BF16) if bf16 else (R.TOL_F32_FWD, R.TOL_F32_GRAD)
        assert rel(nchw(o["y"], C), yr.detach()) < ftol and rel(nchw(o["dx"], C), xd.grad) < gtol
        assert rel(o["dgamma"], gd.grad) < R.TOL_F32_GRAD and rel(o["dbeta"], bd.grad) < R.TOL_F32_GRAD
        if res:
            assert rel(nchw(o["dres"], C), rd.grad) < gtol
        assert rel(o["running_mean"], 0.1 * x.double().mean((0, 2, 3))) < R.TOL_F32_FWD
        if ld > C:      # the owner of a padded tensor writes the zeros the next kernel relies on
            assert not o["y"][..., C:].any() and not o["dx"][..., C:].any()

    _engine_pair(f"bn2 stats / apply / backward C{C} ld{ld}", "bn2_*_kernel, 1190 pixels", fn, verify, K, monkeypatch)


def test_stem7_forward_and_wgrad(K, monkeypatch):
    """nvq_stem7_forward / nvq_stem7_wgrad through nerve_cl._ops.Stem7; bounds: tests/_sr_replay.py TOL_F32_FWD / TOL_F32_GRAD"""
    from nerve_cl import _ops
    import _sr_replay as R
    Co, Hs, Ws = 16, 37, 45
    x, w = rnd(N2, 4, Hs, Ws), rnd(Co, 4, 7, 7) / 14
    wd = w.double().requires_grad_()
    yr = F.conv2d(x.double(), wd, None, stride=2, padding=3)
    dy = rnd(*yr.shape, seed=4)
    yr.backward(dy.double())

    def fn():
        wc = w.cuda().requires_grad_()
        y = _ops.Stem7.apply(to_nhwc(x), wc, F32)
        y.backward(to_nhwc(dy))
        return {"y": y.detach(), "dw": wc.grad}

    def verify(o):
        assert rel(nchw(o["y"]), yr.detach()) < R.TOL_F32_FWD and rel(o["dw"], wd.grad) < R.TOL_F32_GRAD

    _engine_pair("stem7 forward + wgrad", "stem7_wgrad_kernel", fn, verify, K, monkeypatch)


def test_cbam_with_gap_partial_and_the_spatial_conv_gradient(K, monkeypatch):
    """nvq_gap_partial, cbam_channel / pool / spatial_apply and the backward with nvq_cbam_bwd_spatial_conv (the one CBAM launch
    that takes a workspace) through nerve_cl._ops.CBAMFn; bounds of test_cbam_forward_backward (TOL forward, 5e-5 gradients).
    The arg-max plane is int32 and is not poisoned."""
    from nerve_cl import _ops
    C, B = 32, 2
    H, W = HB, WB                   # six nvq_gap_partial blocks and two dca_partial blocks per image
    R_ = C // 16
    x = rnd(B, C, H, W).requires_grad_()
    Pm = {"temporal_aggregator.refine.channel_attention.fc.0.weight": rnd(R_, C, seed=1).requires_grad_(),
          "temporal_aggregator.refine.channel_attention.fc.2.weight": rnd(C, R_, seed=2).requires_grad_(),
          "temporal_aggregator.refine.spatial_attention.conv.weight": (rnd(1, 2, 7, 7, seed=3) * 0.3).requires_grad_()}
    y = sr_oracle.cbam(Pm, x)
    dy = rnd(B, C, H, W, seed=7)
    y.backward(dy)

    def fn():
        xb = to_nhwc(x.detach()).requires_grad_()
        ws_ = [v.detach().cuda().requires_grad_() for v in Pm.values()]
        out = _ops.CBAMFn.apply(xb, *ws_)
        out.backward(to_nhwc(dy))
        return {"y": out.detach(), "dx": xb.grad, "dw1": ws_[0].grad, "dw2": ws_[1].grad, "dw7": ws_[2].grad}

    def verify(o):
        g1, g2, g7 = [v.grad for v in Pm.values()]
        assert rel(nchw(o["y"]), y.detach()) < TOL and rel(nchw(o["dx"]), x.grad) < GRAD_TOL
        assert rel(o["dw1"], g1) < GRAD_TOL and rel(o["dw2"], g2) < GRAD_TOL and rel(o["dw7"], g7) < GRAD_TOL

    _engine_pair("CBAM (gap_partial .. cbam_bwd_spatial_conv)", "C 32, 37 x 41", fn, verify, K, monkeypatch)


def test_cbam_slices_destinations_and_images(K):
    """the CBAM launches one by one, as test_cbam_forward_backward calls them (same bounds: TOL forward, 5e-5 gradients): every
    output in a NaN destination, the result (`out: Sl` of cbam_spatial_apply) at channel 16 of a wider NaN tensor whose other
    channels must still be NaN afterwards, dout (the `Sl` of cbam_bwd_spatial_pre and cbam_bwd_scale) at channel 16 between NaN
    channels, the workspace of
    nvq_cbam_bwd_spatial_conv NaN; the arg-max plane is int32 and zero-filled.  Then image 1 of 3 NaN: the channel attention is
    per image, so images 0 and 2 keep their bits."""
    C, B = 32, 3
    H, W = HB, WB
    R_ = C // 16
    x = rnd(B, C, H, W).requires_grad_()
    Pm = {"temporal_aggregator.refine.channel_attention.fc.0.weight": rnd(R_, C, seed=1).requires_grad_(),
          "temporal_aggregator.refine.channel_attention.fc.2.weight": rnd(C, R_, seed=2).requires_grad_(),
          "temporal_aggregator.refine.spatial_attention.conv.weight": (rnd(1, 2, 7, 7, seed=3) * 0.3).requires_grad_()}
    y = sr_oracle.cbam(Pm, x)
    dy = rnd(B, C, H, W, seed=7)
    y.backward(dy)
    w1, w2, w7 = [v.detach().cuda() for v in Pm.values()]
    nb2 = K.tsum_blocks(H, W)
    assert nb2 == 2

    def run(m, xv=None):
        xv = x.detach() if xv is None else xv
        xb = to_nhwc(xv)
        gp = xv.sum((2, 3)).reshape(B, 1, C).cuda().contiguous()       # (one pooling block per image, as the neighbouring test)
        gap, hid, ca = m.dest(B, C), m.dest(B, R_), m.dest(B, C)
        K.cbam_channel(gp, 1, C, R_, B, H * W, w1, w2, gap, hid, ca)
        sm, sa = m.dest(B, H, W, 2), m.dest(B, H, W)
        amax = torch.zeros(B, H, W, dtype=torch.int32, device="cuda")
        K.cbam_pool(xb, ca, sm, amax)
        cat = m.dest(B, H, W, 16 + C + 16)                              # the result: channels [16, 16 + C) of a NaN tensor
        K.cbam_spatial_apply(xb, ca, sm, w7, sa, K.Sl(cat, C, 16))
        dcat = m.wide(dy, 16 + C + 16, 16)                              # dout: a slice with NaN channels on both sides
        dpre = m.dest(B, H, W)
        K.cbam_bwd_spatial_pre(K.Sl(dcat, C, 16), xb, ca, sa, dpre)
        dsm, dw7 = m.dest(B, H, W, 2), m.dest(1, 2, 7, 7)
        K.cbam_bwd_spatial_conv(dpre, sm, w7, dsm, dw7, m.ws())
        dx, dcap = m.dest(B, H, W, C), m.dest(B, nb2, C)
        K.cbam_bwd_scale(K.Sl(dcat, C, 16), xb, ca, sa, dsm, amax, dx, dcap)
        dw1, dw2, dgp = m.dest(R_, C), m.dest(C, R_), m.dest(B, C)
        K.cbam_bwd_channel(dcap, nb2, C, R_, B, H * W, w1, w2, gap, hid, ca, dw1, dw2, dgp)
        return {"y": cat[..., 16:16 + C].contiguous(), "untouched:y": torch.cat([cat[..., :16], cat[..., 16 + C:]], -1), "ca": ca, "sa": sa, "sm": sm, "dx": dx,
                "dgap_pix": dgp, "dw1": dw1, "dw2": dw2, "dw7": dw7}

    def verify(o):
        g1, g2, g7 = [v.grad for v in Pm.values()]
        assert rel(nchw(o["y"]), y.detach()) < TOL
        assert rel(nchw(o["dx"]) + o["dgap_pix"].cpu()[:, :, None, None], x.grad) < GRAD_TOL
        assert rel(o["dw1"], g1) < GRAD_TOL and rel(o["dw2"], g2) < GRAD_TOL and rel(o["dw7"], g7) < GRAD_TOL

    pair("CBAM launches, slices", "C 32, 37 x 41, 2 dca blocks", run, verify, K)
    clean = run(Mem(K, False))
    xv = x.detach().clone()
    xv[1] = float("nan")
    got = run(Mem(K, True), xv)
    for k in ("y", "ca", "sa", "sm", "dx", "dgap_pix"):
        P.assert_same_bits(clean[k][0], got[k][0], f"CBAM: {k}, image 0")
        P.assert_same_bits(clean[k][2], got[k][2], f"CBAM: {k}, image 2")


def test_losses_metrics_and_flat_reductions(K, monkeypatch):
    """mse_forward, quality_sums, pixel_loss_forward, ssim_forward, the MS-SSIM scale passes, cosine_distill_forward, ewc_penalty
    and bucket_moments: every one reduces through the engine's workspace into a torch.empty output.  Bounds: 2e-5 relative
    (REL of tests/test_metrics_gpu.py) against float64 formulas; SSIM 1e-4 absolute (its hard cap there);
    MS-SSIM 2e-5 absolute against ms_ssim_ref with the five standard weights (VALUE_CAP of tests/test_msssim_gpu.py's
    test_value_and_gradient); ewc 1e-5 (test_ewc_flat_kernels)."""
    from nerve_cl import _engine, metrics, ops
    from test_metrics_gpu import REL, images, pixel_ref, ssim_ref
    from test_msssim_gpu import STANDARD, VALUE_CAP, ms_ssim_ref      # (2e-5 on the value: the fixed ceiling of that file)
    x, y = images((2, 3, 37, 70), 1, zeros=True)
    xm, ym = images((2, 3, 180, 196), 2)
    s, t = torch.randn(2, 32, 9, 14, generator=torch.Generator().manual_seed(3)).cuda(), \
        torch.randn(2, 32, 9, 14, generator=torch.Generator().manual_seed(4)).cuda()
    n = 100_003
    th, st, fi = rnd(n).cuda(), rnd(n, seed=2).cuda(), rnd(n, seed=3).abs().cuda()
    dev = x.device

    def fn():
        out = {"quality_sums": metrics.quality_sums(x, y), "mse": ops.mse_loss(x, y).reshape(1),
               "l1": ops.l1_loss(x, y, reduction="none"), "charbonnier": ops.charbonnier_loss(x, y).reshape(1),
               "ssim": ops.ssim_loss(x, y, reduction="none"), "ms_ssim": ops.ms_ssim_loss(xm, ym, reduction="none"),
               "cosine": ops.cosine_feature_loss(s, t, reduction="none")}
        pen = torch.empty(1, device=dev)
        K.ewc_penalty(th, st, fi, 5000.0, pen, _engine.workspace(dev))
        acc = torch.empty(5, dtype=F64, device=dev)
        K.bucket_moments(th, st, acc, _engine.workspace(dev))
        out["ewc_penalty"], out["bucket_moments"] = pen, acc[:3].clone()
        return out

    def verify(o):
        xd, yd = x.double().flatten(1), y.double().flatten(1)
        d = xd - yd
        want = torch.stack([torch.full((2,), float(xd.shape[1]), dtype=F64, device=dev), xd.sum(1), yd.sum(1), (xd * xd).sum(1),
                            (yd * yd).sum(1), (xd * yd).sum(1), d.abs().sum(1), (d * d).sum(1)], 1)
        assert ((o["quality_sums"] - want).abs() / want.abs()).max().item() <= REL
        assert abs(o["mse"].item() / pixel_ref("mse", x, y, 0).mean().item() - 1) <= REL
        assert ((o["l1"].double() - pixel_ref("l1", x, y, 0)).abs() / pixel_ref("l1", x, y, 0)).max().item() <= REL
        assert abs(o["charbonnier"].item() / pixel_ref("charbonnier", x, y, 1e-3).mean().item() - 1) <= REL
        assert ((1 - o["ssim"].double()) - ssim_ref(x, y)).abs().max().item() <= 1e-4
        cos = 1 - F.cosine_similarity(s.double(), t.double(), dim=1, eps=1e-8).mean((1, 2))
        assert ((o["cosine"].double() - cos).abs() / cos.abs()).max().item() <= REL
        pen = 2500.0 * (fi.double() * (th.double() - st.double()) ** 2).sum()
        assert abs(o["ewc_penalty"].item() - pen.item()) < 1e-5 * abs(pen.item())
        mom = torch.stack([(th.double() * st.double()).sum(), (st.double() ** 2).sum(), (th.double() ** 2).sum()])
        assert ((o["bucket_moments"] - mom).abs() / mom.abs()).max().item() <= REL
        assert ((1 - o["ms_ssim"].double()) - ms_ssim_ref(xm, ym, STANDARD)).abs().max().item() <= VALUE_CAP

    _engine_pair("losses / metrics / ewc / bucket moments", "two-stage reductions through ws", fn, verify, K, monkeypatch)


# =============================================================================== (b) neighbour slices, (c) images, (d) pixels
CONV_FORMS = {
    # name: (cin, coff, ld, cout, k, math, in bf16, out bf16, tile_rows, planar F, bound)
    "conv f32 1x1 40 at 8 in 64": (40, 8, 64, 32, 1, "f32", False, False, 0, 0, TOL),
    "conv f32 3x3 40 at 8 in 64": (40, 8, 64, 32, 3, "f32", False, False, 0, 0, TOL),
    "conv f32 3x3 40 -> 10 (pad4 zeros)": (40, 8, 64, 10, 3, "f32", False, False, 0, 0, TOL),
    "conv bf16-math fp32-stored 3x3 40 at 8 in 64": (40, 8, 64, 32, 3, "bf16", False, False, 0, 0, TOL),
    "conv bf16 3x3 64 at 32 in 128, four-wave": (64, 32, 128, 32, 3, "bf16", True, True, 8, 0, BF16_ONE_ROUNDING),
    "conv bf16 3x3 64 at 32 in 128, eight-wave": (64, 32, 128, 32, 3, "bf16", True, True, 16, 0, BF16_ONE_ROUNDING),
    "conv bf16 3x3 64 at 32 in 128, 32x32x16 (162)": (64, 32, 128, 32, 3, "bf16", True, True, 162, 0, 8e-3),
    "conv bf16 3x3 64 at 32 in 128, 32x32x16 (164)": (64, 32, 128, 32, 3, "bf16", True, True, 164, 0, 8e-3),
    "conv bf16 3x3 96 at 0 in 256, tall tiles": (96, 0, 256, 32, 3, "bf16", True, True, 16, 0, 8e-3),
    "conv bf16 3x3 96 at 0 in 256 -> 64, channel split": (96, 0, 256, 64, 3, "bf16", True, True, 16, 0, 1.2e-2),
    "conv bf16 3x3 96 at 0 in 256, automatic": (96, 0, 256, 32, 3, "bf16", True, True, 0, 0, 8e-3),
    "conv bf16 1x1 96 at 0 in 256 -> 64": (96, 0, 256, 64, 1, "bf16", True, True, 0, 0, BF16_ONE_ROUNDING),
    "conv bf16 1x1 64 at 32 in 128 -> 8": (64, 32, 128, 8, 1, "bf16", True, False, 0, 0, TOL),
    "conv bf16 3x3 slice-planar 96 of 128": (96, 0, 0, 32, 3, "bf16", True, True, 0, 64, 8e-3),
    "conv bf16 1x1 slice-planar 160 of 192 -> 64": (160, 0, 0, 64, 1, "bf16", True, True, 0, 64, BF16_ONE_ROUNDING),
}


def _conv_case(K, name, n=N2, h=H, w=W):
    cin, coff, ld, cout, k, math, in16, out16, rows, planar_F, bound = CONV_FORMS[name]
    x = rnd(n, cin, h, w)
    wt, b = rnd(cout, cin, k, k, scale=0.2), rnd(cout)
    bmath = math == "bf16"
    if bmath:
        x = bf(x)
    mm = K.MATH_BF16 if bmath else K.MATH_F32
    wp = K.conv_pack(wt.cuda(), False, cin, math=mm)
    cst = (cout + 7) // 8 * 8 if out16 else K.pad4(cout)

    def run(m, xv=None, out_fill=None):
        """xv: the input values (NCHW, possibly with NaN pixels / images); every destination is an overwritten one"""
        xv = x if xv is None else xv
        if planar_F:
            xs = planar_input(K, m, xv, cin, planar_F)
        else:
            xs = K.Sl(m.wide(xv, ld, coff, dtype=B16 if in16 else F32), cin, coff)
        out = m.dest(n, h, w, 8 + cst + 8, dtype=B16 if out16 else F32)
        # (no ReLU: max(NaN, 0) is 0 on this hardware, and the bad-pixel checks want to see where a NaN arrives)
        K.conv_forward(xs, wp, b.cuda(), K.Sl(out, cout, 8), k, cout_store=cst, math=mm, tile_rows=rows)
        return {"y": out[..., 8:8 + cout].contiguous(), "pad": out[..., 8 + cout:8 + cst].contiguous(),
                "untouched:y": torch.cat([out[..., :8], out[..., 8 + cst:]], -1)}

    def ref(xv=None):
        return F.conv2d(x if xv is None else xv, bf(wt) if bmath else wt, b, padding=k // 2)

    return dict(run=run, ref=ref, x=x, cout=cout, k=k, bound=bound, cst=cst)


@pytest.mark.parametrize("name", list(CONV_FORMS))
def test_conv_forward_neighbour_slices_and_destination(K, consts, name):
    """(a) + (b) for nvq_conv_forward: the input slice inside a wider tensor of NaN (fp32 cin 40 at 8 in 64: the third K chunk of
    16 reaches 8 channels into the neighbour; bf16 64 at 32 in 128 and 96 at 0 in 256; a slice-planar buffer with an unread
    plane), the output slice inside a NaN tensor.  Bounds: test_conv_forward_bias_relu / test_conv_bf16_forward_bias_relu (TOL),
    test_conv_bf16_stored_input_and_output (5e-3), the eight-wave / 32x32x16 tests (8e-3, 1.2e-2)."""
    c = _conv_case(K, name)
    cin, coff, ld, cout, k, math, in16, out16, rows, planar_F, bound = CONV_FORMS[name]
    if math == "f32":
        r = LF.conv_f32_rule(consts, cout, k, N2, H, W)
        form = f"conv_f32_kernel<{r['form'][0]},{r['form'][1]},{r['form'][2]}>"
    elif rows == 0 and k == 3 and in16 and 16 < cout <= 32:
        r = LF.bf16_auto_rule(consts, cin, cout, H, W)        # the automatic choice, from the mirror of `underfilled`
        form = f"conv_bf16 automatic = tile_rows {r['same_as']}" + (" slice-planar" if planar_F else "")
    else:
        form = f"requested: tile_rows {rows}" + (" slice-planar" if planar_F else "")
    want = c["ref"]()

    def verify(o):
        assert rel(nchw(o["y"]), want) < bound
        assert not o["pad"].float().any()          # the padding up to cout_store is written as zero

    pair(name, form, c["run"], verify, K)


@pytest.mark.parametrize("name", ["conv f32 3x3 40 at 8 in 64", "conv f32 1x1 40 at 8 in 64", "conv bf16 3x3 64 at 32 in 128, four-wave",
                                  "conv bf16 3x3 64 at 32 in 128, eight-wave", "conv bf16 3x3 64 at 32 in 128, 32x32x16 (162)",
                                  "conv bf16 3x3 96 at 0 in 256 -> 64, channel split", "conv bf16 1x1 96 at 0 in 256 -> 64",
                                  "conv bf16 3x3 slice-planar 96 of 128"])
def test_conv_images_are_independent_and_a_bad_pixel_stays_local(K, name):
    """(c): image 1 of 3 all NaN - images 0 and 2 of the output have the bits of the clean call.  (d): one NaN pixel (every
    channel) of image 0 at the corners and on both sides of a tile seam - a 3x3 conv is NaN within the pixel's 3x3 neighbourhood
    (every output channel: the weights are dense), a 1x1 conv at that pixel, and bit-identical everywhere else."""
    c = _conv_case(K, name, n=3)
    clean = images_and_bad_pixels(K, name, lambda m, xv: c["run"](m, xv)["y"], c["x"], c["k"])
    assert rel(nchw(clean), c["ref"]()) < c["bound"]
    print(f"\nPOISON kernel {name:44s} form {'images + 4 bad pixels':40s} bytes {'-':>10s} pass")


DGRAD_FORMS = {
    # name: (cin of the forward = channels of the gradient, cout of the forward, k, math, dy bf16, bound)
    "dgrad f32 3x3 32 -> 64": (64, 32, 3, "f32", False, TOL),
    "dgrad f32 1x1 12 -> 40": (40, 12, 1, "f32", False, TOL),
    "dgrad bf16 3x3 32 -> 96": (96, 32, 3, "bf16", True, TOL),
}


@pytest.mark.parametrize("name", list(DGRAD_FORMS))
def test_conv_input_gradient_via_the_transposed_pack(K, name):
    """the input gradient = the forward kernel with the transposed pack (test_conv_input_gradient_accumulate_mask,
    test_conv_bf16_input_gradient: TOL), overwrite mode into a NaN destination, dy as a slice between NaN channels; images
    independent and one bad pixel local, as for the forward"""
    cin, cout, k, math, dy16, bound = DGRAD_FORMS[name]
    bmath = math == "bf16"
    n = 3
    dy = rnd(n, cout, H, W, seed=3)
    wt = rnd(cout, cin, k, k, scale=0.2)
    if bmath:
        dy = bf(dy)
    mm = K.MATH_BF16 if bmath else K.MATH_F32
    pad = 8 if dy16 else 4
    cs = (cout + pad - 1) // pad * pad
    wp = K.conv_pack(wt.cuda(), True, cs, cin, math=mm)

    def ref(dyv):
        return F.conv_transpose2d(dyv, bf(wt) if bmath else wt, None, padding=k // 2)

    def run(m, dyv=None):
        dyt = m.wide(dy if dyv is None else dyv, 8 + cs + 8, 8, zero_to=8 + cs, dtype=B16 if dy16 else F32)
        out = m.dest(n, H, W, cin + 8)
        K.conv_forward(K.Sl(dyt, cs, 8), wp, None, K.Sl(out, cin, 0), k, cout_store=cin, math=mm)
        return {"dx": out[..., :cin].contiguous(), "untouched:dx": out[..., cin:].contiguous()}

    def verify(o):
        assert rel(nchw(o["dx"]), ref(dy)) < bound

    pair(name, "forward kernel, transposed pack", run, verify, K)
    images_and_bad_pixels(K, name, lambda m, dv: run(m, dv)["dx"], dy, k)


@pytest.mark.parametrize("C,bf16", [(32, False), (64, True)], ids=["fp32-C32", "bf16-C64"])
def test_depthwise_images_and_bad_pixels(K, C, bf16):
    """(c) + (d) for the depthwise 3x3 conv (the tiled fp32 form and the bf16 full-line form); bound TOL / 5e-3 of
    test_depthwise_forward_flip_wgrad / test_dwconv_bf16_full_line_kernels"""
    n = 3
    x, wt = rnd(n, C, H, W), rnd(C, 1, 3, 3)
    wt = torch.where(wt.abs() < 0.05, torch.full_like(wt, 0.05), wt)        # every tap non-zero: the whole 3x3 must turn NaN
    if bf16:
        x = bf(x)
    dt = B16 if bf16 else F32

    def run(m, xv):
        out = m.dest(n, H, W, C, dtype=dt)
        K.dwconv_forward(to_nhwc(xv).to(dt), wt.cuda(), out)
        return out

    clean = images_and_bad_pixels(K, f"depthwise C{C}", run, x, 3)
    assert rel(nchw(clean), F.conv2d(x, wt, None, padding=1, groups=C)) < (BF16_ONE_ROUNDING if bf16 else TOL)
    print(f"\nPOISON kernel {'dwconv_forward C%d' % C:44s} form {'images + 4 bad pixels':40s} bytes {'-':>10s} pass")


@pytest.mark.parametrize("C,mfma,store16", [(32, False, False), (64, True, False), (64, True, True)],
                         ids=["fp32-C32", "mfma-C64-fp32", "mfma-C64-bf16-strip"])
def test_correlation_slices_destination_and_images(K, C, mfma, store16):
    """nvq_correlation_forward and both gradients: x1 as the slice [C, 2C) of a 2C-wide tensor of NaN (also as `other` of the x2
    gradient), x2 (the centre features) as the slice [C, 2C) of a 3C-wide one, corr in a NaN destination, the overwritten
    gradients as slices at channel 8 of NaN tensors; then image 1 of 3 NaN.  Bounds: test_correlation_forward_backward /
    test_correlation_mfma_forward_backward (TOL; 5e-3 for a bf16-stored corr)."""
    B = 3
    x1, x2 = rnd(B, C, H, W).requires_grad_(), rnd(B, C, H, W, seed=3).requires_grad_()
    if mfma:
        x1, x2 = bf(x1.detach()).requires_grad_(), bf(x2.detach()).requires_grad_()
    out = sr_oracle.correlation(x1, x2)
    dy = rnd(B, 81, H, W, seed=5)
    if mfma:
        dy = bf(dy)
    out.backward(dy)
    mm = K.MATH_BF16 if mfma else K.MATH_F32
    fdt = B16 if store16 else F32
    ldc = 128 if store16 else 96

    def run(m, v1=None, v2=None):
        v1, v2 = (x1.detach() if v1 is None else v1), (x2.detach() if v2 is None else v2)
        x1s = K.Sl(m.wide(v1, 2 * C, C, dtype=fdt), C, C)               # x1 (and `other` of the x2 gradient): [C, 2C) of 2C
        al = m.wide(v2, 3 * C, C, dtype=fdt)
        corr = m.dest(B, H, W, ldc, dtype=fdt)
        K.correlation_forward(x1s, K.Sl(al, C, C), corr, math=mm)
        dcorr = to_nhwc(dy, ldc).to(fdt)
        d1 = m.dest(B, H, W, 8 + C + 8)
        K.correlation_backward(1, dcorr, K.Sl(al, C, C), K.Sl(d1, C, 8), False, math=mm)
        d2 = m.dest(B, H, W, 8 + C + 8)
        K.correlation_backward(2, dcorr, x1s, K.Sl(d2, C, 8), False, math=mm)
        return {"corr": corr[..., :81].contiguous(), "corr_pad": corr[..., 81:].contiguous(), "dx1": d1[..., 8:8 + C].contiguous(),
                "dx2": d2[..., 8:8 + C].contiguous(), "untouched:dx1": torch.cat([d1[..., :8], d1[..., 8 + C:]], -1),
                "untouched:dx2": torch.cat([d2[..., :8], d2[..., 8 + C:]], -1)}

    def verify(o):
        assert rel(nchw(o["corr"]), out.detach()) < (BF16_ONE_ROUNDING if store16 else TOL)
        assert not o["corr_pad"].float().any()
        assert rel(nchw(o["dx1"]), x1.grad) < TOL and rel(nchw(o["dx2"]), x2.grad) < TOL

    name = f"correlation forward + gradients C{C} {'mfma' if mfma else 'fp32'}{' bf16-stored' if store16 else ''}"
    pair(name, "strip forms" if store16 else "tile forms", run, verify, K)
    clean = run(Mem(K, False))
    v1, v2 = x1.detach().clone(), x2.detach().clone()
    v1[1], v2[1] = float("nan"), float("nan")
    got = run(Mem(K, True), v1, v2)
    for k in ("corr", "dx1", "dx2"):
        P.assert_same_bits(clean[k][0], got[k][0], f"{name}: {k}, image 0")
        P.assert_same_bits(clean[k][2], got[k][2], f"{name}: {k}, image 2")


@pytest.mark.parametrize("feat16,out16", [(False, False), (True, True)], ids=["fp32", "bf16"])
def test_warp_forward_slices_destination_and_images(K, feat16, out16):
    """nvq_warp_forward of features that are the slice [C, 2C) of a 3C-wide NaN tensor into the slice [2C, 3C) of another, then
    with the FEATURES of image 1 NaN (the flow is a coordinate and stays finite: tests/_poison.py).  A corner outside the image
    is loaded with weight 0 from the image's first pixel (csrc/motion.hip, warp_fwd_kernel): a mask by multiplication, the one
    known exception to the select rule, recorded in DESIGN.md section 30 - a non-finite first pixel of an image would reach
    that image's border pixels.  It reads only the image's own data; with 1.7 px flows every border pixel has such corners, so
    images 0 and 2 show that nothing arrives through another image.  Bound: 5e-5 of test_warp_forward_backward (5e-3 bf16-stored)."""
    C, B = 32, 3
    feat = bf(rnd(B, C, H, W))
    flow = rnd(B, 2, H, W, seed=7) * 1.7
    want = sr_oracle.warp(feat, flow)
    fdt, odt = (B16 if feat16 else F32), (B16 if out16 else F32)

    def run(m, fv=None):
        al = m.dest(B, H, W, 3 * C, dtype=odt)
        fw = m.wide(feat if fv is None else fv, 3 * C, C, dtype=fdt)         # the features: a slice between NaN channels
        K.warp_forward(K.Sl(fw, C, C), to_nhwc(flow, 4), K.Sl(al, C, 2 * C))
        return {"warped": al[..., 2 * C:].contiguous(), "untouched:warped": al[..., :2 * C].contiguous()}

    def verify(o):
        assert rel(nchw(o["warped"]), want) < (BF16_ONE_ROUNDING if out16 else 5e-5)

    pair(f"warp_forward {'bf16' if feat16 else 'fp32'}", f"warp_fwd_kernel<{feat16},{out16}>".lower(), run, verify, K)
    clean = run(Mem(K, False))["warped"]
    fv = feat.clone()
    fv[1] = float("nan")
    got = run(Mem(K, True), fv)["warped"]
    P.assert_same_bits(clean[0], got[0], "warp: image 0")
    P.assert_same_bits(clean[2], got[2], "warp: image 2")


@pytest.mark.parametrize("overwrite,deterministic", [(True, False), (True, True)], ids=["gather-overwrite", "deterministic"])
def test_warp_backward_destinations(K, overwrite, deterministic):
    """nvq_warp_backward(_ex), overwrite mode: dfeat and dflow in NaN destinations, dout and the features each a slice between
    NaN channels (flows of
    0.8 px: every source inside the gather window, so no float atomics and the pair is bit-comparable).  Bounds of
    test_warp_forward_backward: 5e-5 at the features, 2e-4 at the flow.  The gather pass's hit lists are int32 and allocated by
    the wrapper: not poisoned."""
    C, B = 32, 2
    feat = rnd(B, C, H, W).requires_grad_()
    flow = (rnd(B, 2, H, W, seed=2) * 0.8).requires_grad_()
    dy = rnd(B, C, H, W, seed=4)
    sr_oracle.warp(feat, flow).backward(dy)

    def run(m):
        dal = m.wide(dy, 3 * C, 2 * C)
        fw = m.wide(feat.detach(), 3 * C, C)                                 # the features: a slice between NaN channels
        dfeat, dflow = m.dest(B, H, W, C), m.dest(B, H, W, 4)
        K.warp_backward(K.Sl(dal, C, 2 * C), K.Sl(fw, C, C), to_nhwc(flow.detach(), 4), K.Sl(dfeat), dflow,
                        overwrite=overwrite, deterministic=deterministic)
        return {"dfeat": dfeat, "dflow": dflow[..., :2].contiguous(), "dflow_pad": dflow[..., 2:].contiguous()}

    def verify(o):
        assert rel(nchw(o["dfeat"]), feat.grad) < 5e-5 and rel(nchw(o["dflow"]), flow.grad) < 2e-4
        assert not o["dflow_pad"].any()

    pair(f"warp_backward {'deterministic' if deterministic else 'gather, overwrite'}", "gather form", run, verify, K)


@pytest.mark.parametrize("T", [3, 5])
def test_softmax_weighted_sum_destinations_padding_and_images(K, T):
    """nvq_tsum_forward / backward: every output in a NaN destination; the logits' padding channels [T, pad4(T)) are zero by
    contract (the engine's att.4 conv writes them: cout_store = Tp, asserted by tests/test_sr_replay_gpu.py as `logits_pad`).
    Bounds of test_softmax_weighted_sum (TOL; dlogits 5e-5).  Then image 1 of 3 NaN.  37 x 41 = 1517 pixels: two pooling blocks of
    1024 per image, the second ragged."""
    C, B = 32, 3
    H, W = HB, WB
    al = rnd(B, T * C, H, W).requires_grad_()
    lg = (rnd(B, T, H, W, seed=3) * 3).requires_grad_()
    attn = torch.softmax(lg, 1)
    wt = (al.view(B, T, C, H, W) * attn[:, :, None]).sum(1)
    dw = rnd(B, C, H, W, seed=6)
    dgap = rnd(B, C, seed=8) * 0.1
    (wt * (dw + dgap[:, :, None, None])).sum().backward()
    Tp = K.pad4(T)
    nblk = K.tsum_blocks(H, W)

    def run(m, av=None, lv=None):
        alb = to_nhwc(al.detach() if av is None else av)
        lgb = to_nhwc(lg.detach() if lv is None else lv, Tp)
        attn_b, wt_b, gp = m.dest(B, H, W, Tp), m.dest(B, H, W, C), m.dest(B, nblk, C)
        K.tsum_forward(alb, lgb, T, C, attn_b, wt_b, gp)
        dal, dlg = m.dest(B, H, W, T * C), m.dest(B, H, W, Tp)
        K.tsum_backward(to_nhwc(dw), dgap.cuda(), alb, attn_b, T, C, dal, dlg)
        return {"attn": attn_b[..., :T].contiguous(), "weighted": wt_b, "gap_partial": gp, "daligned": dal,
                "dlogits": dlg[..., :T].contiguous(), "dlogits_pad": dlg[..., T:].contiguous()}

    def verify(o):
        assert rel(nchw(o["weighted"]), wt.detach()) < TOL and rel(nchw(o["attn"]), attn.detach()) < TOL
        assert rel(o["gap_partial"].sum(1).cpu(), wt.detach().sum((2, 3))) < TOL
        assert rel(nchw(o["daligned"]), al.grad) < TOL and rel(nchw(o["dlogits"]), lg.grad) < 5e-5
        assert not o["dlogits_pad"].any()

    pair(f"tsum forward + backward T{T}", f"{nblk} pooling blocks per image", run, verify, K)
    clean = run(Mem(K, False))
    av, lv = al.detach().clone(), lg.detach().clone()
    av[1], lv[1] = float("nan"), float("nan")
    got = run(Mem(K, True), av, lv)
    for k in ("attn", "weighted", "gap_partial", "daligned", "dlogits"):
        P.assert_same_bits(clean[k][0], got[k][0], f"tsum T{T}: {k}, image 0")
        P.assert_same_bits(clean[k][2], got[k][2], f"tsum T{T}: {k}, image 2")


def test_upsampler_tail_slices_destination_and_images(K):
    """nvq_upsampler_tail_forward: the input as the slice [32, 96) of a 128-channel bf16 tensor of NaN, out in a NaN destination
    (the pass mask is uint8: not poisoned); bound 2e-5 absolute of test_upsampler_tail_fused_in_the_conv_epilogue.  Then image
    1 of 3 NaN."""
    s, cin, B, T = 2, 64, 3, 3
    U = 3 * s * s
    frames = rnd(B, T, 3, H, W, seed=1).abs()
    x = bf(rnd(B, cin, H, W, seed=2))
    wt, b = rnd(U, cin, 3, 3, scale=0.08, seed=3), rnd(U, seed=4) * 0.1
    wp = K.conv_pack(wt.cuda(), False, cin, math=K.MATH_BF16)
    pre = sr_oracle.bicubic_up(frames[:, T // 2], s) + F.pixel_shuffle(F.conv2d(x, bf(wt), b, padding=1), s)

    def run(m, xv=None):
        xb = m.wide(x if xv is None else xv, 128, 32, dtype=B16)
        out = m.dest(B, 3, H * s, W * s)
        pm = torch.zeros(B, 3, H * s, W * s, dtype=torch.uint8, device="cuda")
        K.upsampler_tail_forward(K.Sl(xb, cin, 32), wp, b.cuda(), frames.cuda(), T // 2, s, out, pm)
        return {"out": out, "passmask": pm}

    def verify(o):
        assert (o["out"].cpu() - pre.clamp(0, 1)).abs().max().item() < 2e-5

    pair("upsampler_tail_forward", "64 at 32 in 128", run, verify, K)
    clean = run(Mem(K, False))["out"]
    xv = x.clone()
    xv[1] = float("nan")
    got = run(Mem(K, True), xv)["out"]
    P.assert_same_bits(clean[0], got[0], "tail: image 0")
    P.assert_same_bits(clean[2], got[2], "tail: image 2")


def test_cast_slice_neighbours_and_destination(K):
    """nerve_cl._ops.cast_slice_: C channels from a slice between NaN channels into a slice of a NaN tensor, fp32 -> bf16 and
    back: exact (a cast), the other channels of the destination untouched"""
    from nerve_cl import _ops
    C = 24
    x = bf(rnd(N2, C, H, W))

    def run(m):
        src = m.wide(x, 48, 8)
        d16 = m.dest(N2, H, W, 40, dtype=B16)
        _ops.cast_slice_(d16, src, C, dst_coff=8, src_coff=8)
        d32 = m.dest(N2, H, W, 32)
        _ops.cast_slice_(d32, d16, C, dst_coff=4, src_coff=8, alpha=0.5)
        return {"bf16": d16[..., 8:8 + C].contiguous(), "untouched:bf16": torch.cat([d16[..., :8], d16[..., 8 + C:]], -1),
                "fp32": d32[..., 4:4 + C].contiguous(), "untouched:fp32": torch.cat([d32[..., :4], d32[..., 4 + C:]], -1)}

    def verify(o):
        assert torch.equal(nchw(o["bf16"]), x) and torch.equal(nchw(o["fp32"]), 0.5 * x)

    pair("cast_slice_", "fp32 -> bf16 -> fp32 slices", run, verify, K)


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
def test_batchnorm_relu_images_in_eval_mode_and_slices(K, training):
    """nvq_bn_apply_relu with a residual, its output a slice of a NaN tensor; in eval mode (running statistics) the images are
    independent: image 1 of 3 NaN.  Bound TOL of test_batchnorm_relu_groups."""
    C, B, G = 32, 1, 3
    x, res = rnd(G, C, H, W) * 1.5 + 0.3, rnd(G, C, H, W, seed=8)
    gamma, beta = 1 + 0.2 * rnd(C), 0.1 * rnd(C, seed=2)
    rm, rv = 0.1 * rnd(C, seed=3), 1 + 0.3 * rnd(C, seed=4)
    want = torch.cat([F.relu(F.batch_norm(x[g:g + 1], rm.clone(), rv.clone(), gamma, beta, training, 0.1, 1e-5)) for g in range(G)]) + res

    def run(m, xv=None):
        xb = to_nhwc(x if xv is None else xv)
        mean, invstd = m.dest(G, C), m.dest(G, C)
        if training:
            K.bn_stats(xb, B, list(range(G)), mean, invstd, None, None, m.ws())
        else:
            K.bn_eval_stats(rm.cuda(), rv.cuda(), G, mean, invstd)
        out = m.dest(G, H, W, 3 * C)
        K.bn_apply_relu(xb, B, mean, invstd, gamma.cuda(), beta.cuda(), to_nhwc(res), K.Sl(out, C, C), G)
        return {"y": out[..., C:2 * C].contiguous(), "untouched:y": torch.cat([out[..., :C], out[..., 2 * C:]], -1)}

    def verify(o):
        assert rel(nchw(o["y"]), want) < TOL

    pair(f"bn_apply_relu {'train' if training else 'eval'}", "residual, output slice", run, verify, K)
    # (with one image per group the batch statistics are per image too, so both modes are per-image here)
    clean = run(Mem(K, False))["y"]
    xv = x.clone()
    xv[1] = float("nan")
    got = run(Mem(K, True), xv)["y"]
    P.assert_same_bits(clean[0], got[0], "bn_apply_relu: image 0")
    P.assert_same_bits(clean[2], got[2], "bn_apply_relu: image 2")
