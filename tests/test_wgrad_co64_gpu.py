"""GPU: the 3x3 weight gradient with 64 output channels per workgroup (wgrad_bf16_kernel<3, true, true, 64, 64, 8>: bf16 x and
dy, cout > 32, eight waves, the x halo tile staged once per 64 co), through the C ABI, against autograd's weight / bias gradient
of F.conv2d on the same bf16 values and against the forced 32-co form (nvq_wgrad_desc::variant = 3).  bf16 x bf16 products are
exact in fp32, so kernel and reference differ by summation order only: the 2e-5 bound of the other weight-gradient tests."""
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

TOL = 2e-5
OLD = 3         # nvq_wgrad_desc::variant: the split kernel with 32 output channels per workgroup

# N, H, W: partial 8x32 tiles both ways and more than one tile per pixel split / a single tile
SIZES = [(2, 13, 37), (1, 8, 32)]
# cin_w, x_ld (stored input channels), cout
CHANNELS = [
    (81, 96, 128),      # a dead 16-ci wave in the second ci chunk
    (128, 128, 81),     # 17 live channels in the second co workgroup: its waves 4-7 are dead
    (192, 192, 64),     # three 64-ci chunks
    (64, 64, 64),       # one chunk each way
    (40, 40, 192),      # cin no multiple of 16, three co workgroups
]


@pytest.fixture(scope="module")
def K():
    if not torch.cuda.is_available():
        pytest.fail("GPU tests need a HIP device")
    from nerve_cl import _nvq
    _nvq.lib()
    return _nvq


def rnd(*shape, seed=0):
    g = torch.Generator().manual_seed(seed + sum(shape))
    return torch.rand(*shape, generator=g) * 2 - 1


def nhwc_bf16(x, ld, coff=0, fill=0.75):
    """CPU NCHW -> cuda bf16 [N,H,W,ld] with the channels at [coff, coff+C); `fill` everywhere else (must not be summed)."""
    n, c, h, w = x.shape
    buf = torch.full((n, h, w, ld), fill, dtype=torch.float32)
    buf[..., coff:coff + c] = x.permute(0, 2, 3, 1)
    return buf.bfloat16().cuda()


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


@functools.lru_cache(maxsize=None)
def case(cin_w, x_ld, cout, N, H, W):
    """bf16-valued x (x_ld stored channels, the first cin_w get a gradient) and dy, and autograd's gradients: computed once."""
    x = rnd(N, x_ld, H, W).bfloat16().float()
    dy = rnd(N, cout, H, W, seed=3).bfloat16().float()
    w = torch.zeros(cout, cin_w, 3, 3, requires_grad=True)
    F.conv2d(x[:, :cin_w], w, None, padding=1).backward(dy)
    return x, dy, w.grad, dy.sum((0, 2, 3))


def dy_ld(cout):
    return 8 + (cout + 7) // 8 * 8      # the slice at channel 8, readable up to a multiple of 8 channels


def run(K, x, cin_w, dy, variant, *, x_pad=0, alpha=1.0, accumulate=False, init=0.0, defer=None, ws=None):
    cout = dy.shape[1]
    xs = nhwc_bf16(x, x.shape[1] + x_pad, x_pad)
    ds = nhwc_bf16(dy, dy_ld(cout), 8)
    dw = torch.full((cout, cin_w, 3, 3), init, device="cuda")
    db = torch.full((cout,), init, device="cuda")
    ws = ws if ws is not None else torch.empty(K.wgrad_workspace_bytes() // 4, dtype=torch.float32, device="cuda")
    K.conv_wgrad(K.Sl(xs, x.shape[1], x_pad), cin_w, K.Sl(ds, cout, 8), dw, db, ws, 3, alpha=alpha, accumulate=accumulate,
                 math=K.MATH_BF16, variant=variant, defer=defer)
    return dw, db


@pytest.mark.parametrize("N,H,W", SIZES)
@pytest.mark.parametrize("cin_w,x_ld,cout", CHANNELS)
def test_wgrad_3x3_64_co_per_workgroup(K, cin_w, x_ld, cout, N, H, W):
    x, dy, gw, gb = case(cin_w, x_ld, cout, N, H, W)
    dw, db = run(K, x, cin_w, dy, 0)
    assert rel(dw, gw) < TOL and rel(db, gb) < TOL
    dw32, db32 = run(K, x, cin_w, dy, OLD)
    assert rel(dw32, gw) < TOL and rel(db32, gb) < TOL
    assert rel(dw, dw32) < TOL and rel(db, db32) < TOL


def test_wgrad_3x3_64_co_alpha(K):
    x, dy, gw, gb = case(81, 96, 128, *SIZES[0])
    dw, db = run(K, x, 81, dy, 0, alpha=0.25, init=7.0)
    assert rel(dw, 0.25 * gw) < TOL and rel(db, 0.25 * gb) < TOL


def test_wgrad_3x3_64_co_accumulate(K):
    x, dy, gw, gb = case(128, 128, 81, *SIZES[0])
    dw, db = run(K, x, 128, dy, 0, alpha=0.5, accumulate=True, init=0.5)
    assert rel(dw, 0.5 * gw + 0.5) < TOL and rel(db, 0.5 * gb + 0.5) < TOL


def test_wgrad_3x3_64_co_partial_and_batched_reduce(K):
    """nvq_conv_wgrad_partial + nvq_wgrad_reduce_batch: the same sums in the same order as nvq_conv_wgrad."""
    x, dy, gw, gb = case(192, 192, 64, *SIZES[0])
    dw0, db0 = run(K, x, 192, dy, 0)
    jobs = []
    dw1, db1 = run(K, x, 192, dy, 0, defer=jobs)
    assert len(jobs) == 1 and dw1.abs().max().item() == 0        # nothing reduced yet
    K.wgrad_reduce_batch(jobs)
    assert torch.equal(dw0, dw1) and torch.equal(db0, db1)
    assert rel(dw1, gw) < TOL and rel(db1, gb) < TOL


def test_wgrad_3x3_64_co_input_slice_of_a_wider_buffer(K):
    x, dy, gw, gb = case(64, 64, 64, *SIZES[0])
    dw, db = run(K, x, 64, dy, 0, x_pad=16)
    assert rel(dw, gw) < TOL and rel(db, gb) < TOL
    dw32, db32 = run(K, x, 64, dy, OLD, x_pad=16)
    assert rel(dw, dw32) < TOL and rel(db, db32) < TOL
