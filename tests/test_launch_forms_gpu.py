"""GPU: the kernel forms that only large launches select, at the smallest shapes that select them, each against a float64 CPU
reference of the same operation (torch.nn.functional).  The shapes come from the table of tests/test_launch_forms_cpu.py,
which proves on the CPU that every row sits on the intended side of its host rule.

fp32 kernels: TOL = 2e-5 of the reference's maximum (summation order only).  bf16 forms: the same bound against the float64
convolution of the bf16-rounded operands (bf16 x bf16 products are exact in fp32), as the neighbouring tests of
tests/test_kernels_gpu.py.  A bf16-STORED result is one more rounding: 2^-8 of the maximum.

References are computed once, for the largest batch, and sliced: the convolutions are per-image."""
import pytest
import torch
import torch.nn.functional as F

from test_launch_forms_cpu import BY_NAME, CASES, CIN, FH, FW

pytestmark = pytest.mark.gpu

TOL = 2e-5
TOL_BF16_STORED = 2.0 ** -8
FILL = 7.0


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


def bf(x):
    return x.bfloat16().float()


def to_nhwc(x, ld=None, coff=0, fill=0.0):
    n, c, h, w = x.shape
    ld = ld or c
    buf = torch.full((n, h, w, ld), fill, dtype=torch.float32)
    buf[..., coff:coff + c] = x.permute(0, 2, 3, 1)
    return buf.cuda()


def from_nhwc(buf, c=None, coff=0):
    c = buf.shape[-1] - coff if c is None else c
    return buf[..., coff:coff + c].permute(0, 3, 1, 2).contiguous().cpu()


def rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


def ws_tensor(K):
    return torch.empty(K.wgrad_workspace_bytes() // 4 + (1 << 20), dtype=torch.float32, device="cuda")


def row(name):
    return BY_NAME[name]


# ----------------------------------------------------------------------------- (a), (c): forward, bias + ReLU, cin 40
NMAX, CMAX = 8, 128


@pytest.fixture(scope="module")
def cache():
    """operands, float64 references and launch results shared by the tests of this file; dropped with the module.
    ("fwd", ks) -> (x, w, b, reference of the N = 8, cout = 128 layer, x on the device); ("out", ks, cout, N) -> the output buffer
    of that launch; ("wgrad", row name) -> operands and reference of a weight-gradient row"""
    d = {}
    yield d
    d.clear()


def fwd_operands(cache, ks):
    if ("fwd", ks) not in cache:
        x, w, b = rnd(NMAX, CIN, FH, FW, seed=ks), rnd(CMAX, CIN, ks, ks, seed=ks, scale=0.2), rnd(CMAX, seed=ks)
        ref = F.relu(F.conv2d(x.double(), w.double(), b.double(), padding=ks // 2))
        cache[("fwd", ks)] = (x, w, b, ref, to_nhwc(x))
    return cache[("fwd", ks)]


def stored(cout):
    """the partly filled slabs (48 of 64, 24 of 32) also store one group of padding channels"""
    return cout + 4 if cout in (48, 24) else cout


def fwd_launch(K, cache, ks, cout, N):
    """relu(conv(x[:N], w[:cout]) + b[:cout]) into a buffer filled with FILL, 4 channels wider than cout_store"""
    if ("out", ks, cout, N) not in cache:
        _, w, b, _, xin = fwd_operands(cache, ks)
        out = torch.full((N, FH, FW, stored(cout) + 4), FILL, device="cuda")
        K.conv_forward(K.Sl(xin[:N]), K.conv_pack(w[:cout].cuda(), False, CIN), b[:cout].cuda(), K.Sl(out, cout, 0), ks, relu=True,
                       cout_store=stored(cout))
        cache[("out", ks, cout, N)] = out
    return cache[("out", ks, cout, N)]


FWD_ROWS = [r for r in CASES if r["name"].startswith("fwd_")]


@pytest.mark.parametrize("r", FWD_ROWS, ids=[r["name"] for r in FWD_ROWS])
def test_conv_forward_form_against_float64(K, cache, r):
    """every size-selected conv_f32_kernel<NB,KS,GS> (the row's want["form"]) on a frame ragged on both edges, with a ragged
    third K chunk; cout 48 / 24 leave the slab partly filled, cout 128 has a second slab (blockIdx.y = 1)"""
    ks, cout, N = r["ks"], r["cout"], r["N"]
    assert (r["H"], r["W"]) == (FH, FW)
    ref = fwd_operands(cache, ks)[3][:N, :cout]
    out = fwd_launch(K, cache, ks, cout, N)
    cst = stored(cout)
    err = rel(from_nhwc(out, cout), ref)
    print(f"{r['name']} form {r['want']['form']}: {err:.2e}")
    assert err < TOL
    if cst > cout:
        assert out[..., cout:cst].abs().max().item() == 0.0      # padded channels written as zero
    assert (out[..., cst:] == FILL).all()                         # nothing beyond cout_store touched


@pytest.mark.parametrize("name", ["edge_g129", "edge_g257"])
def test_conv_forward_at_the_edges_of_the_rule(K, name):
    """one-tile-high strips of 129 tiles (the first gs = 2 launch) and 257 tiles (the first gs = 1 launch)"""
    r = row(name)
    cin, cout, ks, N, H, W = 16, r["cout"], r["ks"], r["N"], r["H"], r["W"]
    x, w, b = rnd(N, cin, H, W), rnd(cout, cin, ks, ks, scale=0.2), rnd(cout)
    ref = F.relu(F.conv2d(x.double(), w.double(), b.double(), padding=ks // 2))
    out = torch.full((N, H, W, cout + 4), FILL, device="cuda")
    K.conv_forward(K.Sl(to_nhwc(x)), K.conv_pack(w.cuda(), False, cin), b.cuda(), K.Sl(out, cout, 0), ks, relu=True)
    assert rel(from_nhwc(out, cout), ref) < TOL
    assert (out[..., cout:] == FILL).all()


@pytest.mark.parametrize("ks", [1, 3])
@pytest.mark.parametrize("cout", [64, 128, 32])
def test_one_image_has_the_same_bits_in_every_form(K, cache, cout, ks):
    """Image 0 of the N = 8, N = 4 (cout 128: also N = 2) and N = 1 launches: <4,KS,1> / <2,KS,2> / <1,KS,4> for 64 and 128
    output channels, <2,KS,1> / <1,KS,2> for 32.  The forms split the output channels of a slab over workgroups, never the sum
    of one output: K chunks, taps and the four k of an MFMA come in the same order, so the results are bit-identical."""
    batches = (8, 4, 2, 1) if cout == 128 else (8, 4, 1)
    forms = {row(f"fwd_k{ks}_c{cout}_n{n}")["want"]["form"] for n in batches}
    assert len(forms) == (3 if cout >= 64 else 2)
    one = fwd_launch(K, cache, ks, cout, 1)
    for n in batches[:-1]:
        assert torch.equal(fwd_launch(K, cache, ks, cout, n)[:1], one), (cout, ks, n)


# ----------------------------------------------------------------------------- (b): epilogues on <4,KS,1> / <2,KS,1>
def test_lff_epilogue_on_the_large_form(K):
    """out = 0.2 * (conv1x1(cat) + b) + cat[:, :F] written into a channel slice (conv_f32_kernel<4,1,1>; 104 input channels:
    six K chunks and a half)"""
    r = row("epi_lff")
    N, H, W, Fc, CAT = r["N"], r["H"], r["W"], r["cout"], 104
    cat, w, b = rnd(N, CAT, H, W), rnd(Fc, CAT, 1, 1, scale=0.1), rnd(Fc)
    ref = F.conv2d(cat.double(), w.double(), b.double()) * 0.2 + cat[:, :Fc].double()
    catb = to_nhwc(cat)
    out = torch.zeros(N, H, W, CAT, device="cuda")
    K.conv_forward(K.Sl(catb), K.conv_pack(w.cuda(), False, CAT), b.cuda(), K.Sl(out, Fc, 32), 1, alpha=0.2, res=K.Sl(catb, Fc, 0))
    assert rel(from_nhwc(out, Fc, 32), ref) < TOL
    assert out[..., :32].abs().max().item() == 0 and out[..., 32 + Fc:].abs().max().item() == 0


def test_out2_and_residual_after_relu_on_the_large_form(K, cache):
    """out2 = relu(conv + b), out = out2 + centre (conv_f32_kernel<4,3,1>)"""
    r = row("epi_out2")
    N, H, W, Fc, ks = r["N"], r["H"], r["W"], r["cout"], r["ks"]
    _, w, b, ref, xin = fwd_operands(cache, ks)
    ref = ref[:N, :Fc]
    cen = rnd(N, Fc, H, W, seed=5)
    out, out2 = torch.full((N, H, W, Fc + 4), FILL, device="cuda"), torch.full((N, H, W, Fc + 4), FILL, device="cuda")
    K.conv_forward(K.Sl(xin[:N]), K.conv_pack(w[:Fc].cuda(), False, CIN), b[:Fc].cuda(), K.Sl(out, Fc, 0), ks, relu=True,
                   out2=K.Sl(out2, Fc, 0), res=K.Sl(to_nhwc(cen, 96, 32), Fc, 32))
    assert rel(from_nhwc(out2, Fc), ref) < TOL
    assert rel(from_nhwc(out, Fc), ref + cen.double()) < TOL
    assert (out[..., Fc:] == FILL).all() and (out2[..., Fc:] == FILL).all()


@pytest.mark.parametrize("ks", [1, 3])
@pytest.mark.parametrize("cdx,cdy", [(64, 40), (32, 64)])
def test_input_gradient_accumulate_mask_on_the_large_forms(K, cdx, cdy, ks):
    """The input gradient = the forward kernel with the transposed pack, `accumulate` and a ReLU mask on a channel range:
    a cdy-channel gradient into cdx channels, so that both slab widths run (64: <4,KS,1>, 32: <2,KS,1>)."""
    r = row(f"dgrad_k{ks}_{cdx}_from_{cdy}")
    assert r["cout"] == cdx
    N, H, W = r["N"], r["H"], r["W"]
    w = rnd(cdy, cdx, ks, ks, scale=0.2)                 # the forward layer's weight: cdx -> cdy channels
    dy = rnd(N, cdy, H, W, seed=3)
    old, act = rnd(N, cdx, H, W, seed=9), rnd(N, cdx, H, W, seed=11)
    c0, c1 = (cdx // 8) * 4, cdx
    want = torch.nn.grad.conv2d_input((N, cdx, H, W), w.double(), dy.double(), padding=ks // 2) + old.double()
    m = torch.ones_like(want)
    m[:, c0:c1] = (act[:, c0:c1] > 0).double()
    want = want * m
    out = to_nhwc(old, cdx + 4, fill=FILL)
    K.conv_forward(K.Sl(to_nhwc(dy)), K.conv_pack(w.cuda(), True, cdy, cdx), None, K.Sl(out, cdx, 0), ks, accumulate=True,
                   mask=K.Sl(to_nhwc(act)), mask_c0=c0, mask_c1=c1)
    assert rel(from_nhwc(out, cdx), want) < TOL
    assert (out[..., cdx:] == FILL).all()


# ----------------------------------------------------------------------------- (d): fp32 weight gradient, 288 tiles
def wgrad_case(K, cache, name):
    """(operands on the device, float64 dw / db of 0.5 * conv) of a weight-gradient row, computed once"""
    if ("wgrad", name) not in cache:
        r = row(name)
        cin, cs, cout, ks, N, H, W = r["cin_w"], r["cin_store"], r["cout"], r["ks"], r["N"], r["H"], r["W"]
        x, dy = rnd(N, cin, H, W, seed=1), rnd(N, cout, H, W, seed=3)
        dw = 0.5 * torch.nn.grad.conv2d_weight(x.double(), (cout, cin, ks, ks), dy.double(), padding=ks // 2)
        db = 0.5 * dy.double().sum((0, 2, 3))
        cache[("wgrad", name)] = (K.Sl(to_nhwc(x, cs)), K.Sl(to_nhwc(dy, cout + 4), cout, 0), dw, db)
    return cache[("wgrad", name)]


@pytest.mark.parametrize("accumulate", [False, True], ids=["overwrite", "accumulate"])
@pytest.mark.parametrize("name", ["wgrad_32_32_k3", "wgrad_64_64_k3", "wgrad_81_128_k1"])
def test_conv_weight_gradient_with_many_tiles_per_split(K, cache, name, accumulate):
    """N = 8 frames = 288 tiles: 288 splits of one tile (the reduce's four-chain loop, five trips of the bias blocks' lane loop),
    128 splits of 2 or 3 tiles, 40 splits of 7 or 8 tiles (81 real input channels stored as 96); bias gradient, alpha = 0.5"""
    r = row(name)
    cin, cout, ks = r["cin_w"], r["cout"], r["ks"]
    xs, dys, dw_ref, db_ref = wgrad_case(K, cache, name)
    dw0, db0 = rnd(cout, cin, ks, ks, seed=21), rnd(cout, seed=22)
    dw, db = dw0.cuda(), db0.cuda()
    K.conv_wgrad(xs, cin, dys, dw, db, ws_tensor(K), ks, alpha=0.5, accumulate=accumulate)
    if accumulate:
        dw_ref, db_ref = dw_ref + dw0.double(), db_ref + db0.double()
    e_w, e_b = rel(dw, dw_ref), rel(db, db_ref)
    print(f"{name} nsplit {r['want']['nsplit']}: dw {e_w:.2e} db {e_b:.2e}")
    assert e_w < TOL and e_b < TOL


def test_conv_weight_gradient_in_two_halves_at_128_splits(K, cache):
    """nvq_conv_wgrad_partial + nvq_wgrad_reduce_batch on the 64 -> 64 case: the same bits as the one-call form"""
    name = "wgrad_64_64_k3"
    r = row(name)
    cin, cout, ks = r["cin_w"], r["cout"], r["ks"]
    xs, dys, dw_ref, db_ref = wgrad_case(K, cache, name)
    mk = lambda: (torch.full((cout, cin, ks, ks), 0.5, device="cuda"), torch.full((cout,), -0.25, device="cuda"))   # noqa: E731
    for accumulate in (False, True):
        dw0, db0 = mk()
        K.conv_wgrad(xs, cin, dys, dw0, db0, ws_tensor(K), ks, alpha=0.5, accumulate=accumulate)
        dw1, db1 = mk()
        jobs = []
        K.conv_wgrad(xs, cin, dys, dw1, db1, ws_tensor(K), ks, alpha=0.5, accumulate=accumulate, defer=jobs)
        assert len(jobs) == 1 and torch.equal(dw1, torch.full_like(dw1, 0.5))      # nothing reduced yet
        K.wgrad_reduce_batch(jobs)
        assert torch.equal(dw0, dw1) and torch.equal(db0, db1)
    assert rel(dw0 - 0.5, dw_ref) < TOL


# ----------------------------------------------------------------------------- (e): 7x7 stride-2 stem
@pytest.mark.parametrize("name", ["stem_co64", "stem_co72"])
def test_stem_with_two_tiles_per_workgroup_and_a_second_channel_pass(name):
    """_ops.Stem7 at 3 x 149x149: 300 tiles on 256 weight-gradient workgroups (44 take a second tile, the partial reduce sees
    256 rows = four trips of its lane loop).  Co = 72: the second 64-channel pass of the forward and of the weight gradient, with
    8 live channels.  Forward, weight gradient from an fp32 and from a bf16 dy, and (Co = 64) the sink's dframe / dmask.
    nvq_stem7_dgrad takes 16 .. 64 channels in multiples of 16 (tests/test_fr_input_grad_cpu.py): Co = 72 has no sink here."""
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device")
    from nerve_cl import _ops
    r = row(name)
    Co, N, H, W = r["Co"], r["N"], r["H"], r["W"]
    OH, OW = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    x, w, dy = rnd(N, 4, H, W), rnd(Co, 4, 7, 7, scale=196 ** -0.5), rnd(N, Co, OH, OW, seed=4)
    y_ref = F.conv2d(x.double(), w.double(), None, stride=2, padding=3)
    x4 = to_nhwc(x)
    sink = None
    if Co <= 64:
        base_f, base_m = rnd(N, 3, H, W, seed=6), rnd(N, 1, H, W, seed=7)
        sink = _ops.InputGradSink(base_f.cuda(), None, base_m.cuda())
    wg = w.cuda().requires_grad_()
    y = _ops.Stem7.apply(x4, wg, torch.float32, sink)
    assert y.shape == (N, OH, OW, Co)
    assert rel(from_nhwc(y), y_ref) < TOL
    y.backward(to_nhwc(dy))
    assert rel(wg.grad, torch.nn.grad.conv2d_weight(x.double(), w.shape, dy.double(), stride=2, padding=3)) < TOL
    if sink is not None:
        dx = torch.nn.grad.conv2d_input((N, 4, H, W), w.double(), dy.double(), stride=2, padding=3)
        assert rel(sink.dframe, dx[:, :3] + base_f.double()) < TOL
        assert rel(sink.dmask, dx[:, 3:] + base_m.double()) < TOL
    # bf16-stored output and gradient: the same fp32 sums rounded once; the weight gradient of the rounded dy
    wg16 = w.cuda().requires_grad_()
    y16 = _ops.Stem7.apply(x4, wg16, torch.bfloat16)
    assert y16.dtype == torch.bfloat16 and rel(from_nhwc(y16.float()), y_ref) < TOL_BF16_STORED
    dy16 = to_nhwc(dy).bfloat16()
    y16.backward(dy16)
    assert rel(wg16.grad, torch.nn.grad.conv2d_weight(x.double(), w.shape, bf(dy).double(), stride=2, padding=3)) < TOL


# ----------------------------------------------------------------------------- (f): depthwise weight gradient
@pytest.mark.parametrize("name", ["dw_f32_c32", "dw_bf16_c64"])
def test_depthwise_weight_gradient_with_two_tiles_per_workgroup(K, name):
    """2 x 129x481 = 544 tiles on 512 persistent workgroups, partial reduce over 512 rows: the fp32 tiled form (C = 32) and the
    bf16 full-line form (C = 64, x and dy stored as bf16) against float64 autograd of F.conv2d(groups=C)"""
    r = row(name)
    C, N, H, W, b16 = r["C"], r["N"], r["H"], r["W"], r["bf16"]
    x, dy = rnd(N, C, H, W) * 1.5 + 0.3, rnd(N, C, H, W, seed=6)
    if b16:
        x, dy = bf(x), bf(dy)
    w = rnd(C, 1, 3, 3).double().requires_grad_()
    F.conv2d(x.double(), w, None, padding=1, groups=C).backward(dy.double())
    xs, ds = to_nhwc(x), to_nhwc(dy)
    if b16:
        xs, ds = xs.bfloat16(), ds.bfloat16()
    dw = torch.full((C, 1, 3, 3), FILL, device="cuda")
    K.dwconv_wgrad(xs, ds, dw, ws_tensor(K))
    assert rel(dw, w.grad) < TOL
    dw2 = torch.full((C, 1, 3, 3), 0.5, device="cuda")
    K.dwconv_wgrad(xs, ds, dw2, ws_tensor(K), accumulate=True)
    assert rel(dw2, w.grad + 0.5) < TOL


# ----------------------------------------------------------------------------- (g): bf16 automatic choice
@pytest.mark.parametrize("name", ["auto_64_32_128x128", "auto_64_32_112x128", "auto_160_32_128x128"])
def test_conv_bf16_automatic_choice_on_both_sides_of_the_rule(K, name):
    """3x3, bf16-stored input, cout 32, tile_rows = 0: an image of 32 16x32 tiles is not underfilled and takes the 32x32x16 form
    (cin <= 128; tile_rows 162) or the eight-wave 16x32-tile form (tile_rows 16); 28 tiles are underfilled and take the four-wave
    8x32-tile kernel (tile_rows 8).  Bit-identical to the forced form, within TOL of the float64 convolution of the same bf16
    values, and - the rule looks at ONE image - image 0 has the same bits alone and in a batch of three."""
    r = row(name)
    cin, cout, H, W, forced = r["cin"], r["cout"], r["H"], r["W"], r["want"]["same_as"]
    N = 3
    x, w, b = bf(rnd(N, cin, H, W, seed=5)), rnd(cout, cin, 3, 3, scale=0.1), rnd(cout, seed=2)
    ref = F.relu(F.conv2d(x.double(), bf(w).double(), b.double(), padding=1))
    xin = to_nhwc(x).bfloat16()
    wp = K.conv_pack(w.cuda(), False, cin, math=K.MATH_BF16)

    def run(n, rows):
        out = torch.full((n, H, W, cout + 4), FILL, device="cuda")
        K.conv_forward(K.Sl(xin[:n]), wp, b.cuda(), K.Sl(out, cout, 0), 3, relu=True, math=K.MATH_BF16, tile_rows=rows)
        assert (out[..., cout:] == FILL).all()
        return out

    auto3, forced3, auto1 = run(3, 0), run(3, forced), run(1, 0)
    assert torch.equal(auto3, forced3)
    assert torch.equal(auto3[:1], auto1)
    assert rel(from_nhwc(auto3, cout), ref) < TOL


# ----------------------------------------------------------------------------- (h): the networks, where the forms differ
def _randomise_running_statistics(net, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for n, b in net.named_buffers():
            if n.endswith("running_mean"):
                b.copy_((0.1 * torch.randn(b.shape, generator=g)).to(b.device))
            elif n.endswith("running_var"):
                b.copy_((0.5 + torch.rand(b.shape, generator=g)).to(b.device))


def test_sr_net_clip_does_not_depend_on_the_batch_at_64x64():
    """SuperResolutionNet(3, 2, 64, 1, 1), eval, fp32 math, 64x64 clips: alone, a clip's 64 -> 64 3x3 layers run
    conv_f32_kernel<1,3,4> (3 frames x 16 tiles = 48 workgroups' worth), in a batch of 8 <4,3,1> (384) - rows net_sr_b1 /
    net_sr_b8.  Eval mode has no reduction over the batch, so the clip's output has the same bits either way."""
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device")
    from nerve_cl import _nvq
    from nerve_cl.models import SuperResolutionNet
    one, eight = row("net_sr_b1"), row("net_sr_b8")
    B, T, H, W = eight["N"] // 3, 3, eight["H"], eight["W"]
    assert one["N"] == T and (one["H"], one["W"]) == (H, W) and B == 8
    torch.manual_seed(3)
    net = SuperResolutionNet(3, 2, one["cout"], 1, 1).cuda().eval()
    net.math_mode, net.bf16_activations = _nvq.MATH_F32, False
    _randomise_running_statistics(net, 4)
    g = torch.Generator(device="cuda").manual_seed(5)
    x = torch.rand(B, T, 3, H, W, device="cuda", generator=g)
    with torch.no_grad():
        both, again = net(x), net(x)
        assert both.shape == (B, 3, 2 * H, 2 * W) and torch.isfinite(both).all()
        assert torch.equal(both, again)
        for k in (0, B - 1):
            assert torch.equal(both[k:k + 1], net(x[k:k + 1])), k


def test_frame_recovery_net_clip_does_not_depend_on_the_batch_at_64x96():
    """FrameRecoveryNet(3, 16, 2), eval, fp32 math, 64x96: B = 1 against B = 8"""
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device")
    from nerve_cl import _nvq
    from nerve_cl.models import FrameRecoveryNet
    B, T, H, W = 8, 2, 64, 96
    torch.manual_seed(6)
    net = FrameRecoveryNet(3, 16, T).cuda().eval()
    net.math_mode, net.bf16_activations = _nvq.MATH_F32, False
    _randomise_running_statistics(net, 7)
    g = torch.Generator(device="cuda").manual_seed(8)
    frame = torch.rand(B, 3, H, W, device="cuda", generator=g)
    refs = torch.rand(B, T, 3, H, W, device="cuda", generator=g)
    mask = torch.zeros(B, 1, H, W, device="cuda")
    mask[:, :, H // 4:H // 4 + H // 2, W // 3:W // 3 + W // 2] = 1.0
    frame = frame * (1 - mask)
    with torch.no_grad():
        both, again = net(frame, refs, mask), net(frame, refs, mask)
        assert both.shape == (B, 3, H, W) and torch.isfinite(both).all()
        assert torch.equal(both, again)
        for k in (0, B - 1):
            assert torch.equal(both[k:k + 1], net(frame[k:k + 1], refs[k:k + 1], mask[k:k + 1])), k
