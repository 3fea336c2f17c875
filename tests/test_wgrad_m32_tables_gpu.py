"""GPU: the all-input-channel 3x3 weight gradient (wgrad_m32.hip) under its per-NCI job tables.  Every number of 32-channel
input blocks the kernel is built for (NCI = 3 .. 6: cin 96 .. 192 behind a 64-channel leading tensor, cin 96 .. 160 behind a
32-channel one) has a table of its own that says which wave accumulates which (block, tap) rectangle; a slab that no wave
owns, or that two own, shows as a wrong dW.  Against autograd's weight / bias gradient of F.conv2d on the same bf16 values,
against the (pixel split, ci chunk) kernel, with alpha / accumulate, and twice for determinism."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

TOL = 2e-5      # fp32 accumulation of exact bf16 products vs the fp32 CPU reference (summation order only)

# (N, H, W): ragged in both directions with fewer tiles than workgroups (some workgroups have no tile); odd unit counts;
# 550 tiles = two to three per workgroup, so the persistent loop and the ring slots turn over
GEOMETRIES = [(1, 9, 33), (4, 45, 70), (2, 100, 330)]
CHANNELS = [(64, 96), (64, 128), (64, 160), (64, 192), (32, 96), (32, 128), (32, 160)]


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


def bf(x):
    return x.bfloat16().float()


def nhwc_bf16(x, ld=None, coff=0):
    n, c, h, w = x.shape
    buf = torch.zeros(n, h, w, ld or c)
    buf[..., coff:coff + c] = x.permute(0, 2, 3, 1)
    return buf.cuda().bfloat16()


def rel(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item()


@pytest.mark.parametrize("N,H,W", GEOMETRIES)
@pytest.mark.parametrize("Fc,cin", CHANNELS)
def test_all_input_channel_weight_gradient_job_tables(K, Fc, cin, N, H, W):
    x, dy = bf(rnd(N, cin, H, W)), bf(rnd(N, 32, H, W, seed=3))
    w = rnd(32, cin, 3, 3).requires_grad_()
    F.conv2d(x, w, None, padding=1).backward(dy)
    dw_ref, db_ref = w.grad, dy.sum((0, 2, 3))
    cat = K.CatBuf("cuda", N, H, W, Fc, (cin - Fc) // 32 + 1, 256, torch.bfloat16, planar=True)
    xn = nhwc_bf16(x)
    cat.lead.copy_(xn[..., :Fc])
    for j in range((cin - Fc) // 32):
        cat.slices[j].copy_(xn[..., Fc + 32 * j:Fc + 32 * (j + 1)])
    ds = nhwc_bf16(dy, 40, 8)
    ws = torch.empty(K.wgrad_workspace_bytes() // 4 + (1 << 20), dtype=torch.float32, device="cuda")

    def run(variant):
        dw, db = torch.full((32, cin, 3, 3), 7.0, device="cuda"), torch.full((32,), 7.0, device="cuda")
        K.conv_wgrad(cat.inp(cin), cin, K.Sl(ds, 32, 8), dw, db, ws, 3, math=K.MATH_BF16, variant=variant)
        return dw, db

    dw, db = run(2)
    e_ref = (rel(dw, dw_ref), rel(db, db_ref))
    dw1, db1 = run(1)
    e_split = (rel(dw, dw1), rel(db, db1))
    dw2, db2 = run(2)
    dwa, dba = dw.clone(), db.clone()
    K.conv_wgrad(cat.inp(cin), cin, K.Sl(ds, 32, 8), dwa, dba, ws, 3, alpha=0.5, accumulate=True, math=K.MATH_BF16, variant=2)
    e_acc = (rel(dwa, 1.5 * dw_ref), rel(dba, 1.5 * db_ref))
    print(f"F {Fc} cin {cin} {N}x{H}x{W}: vs autograd {e_ref}, vs split kernel {e_split}, alpha/accumulate {e_acc}")
    assert max(e_ref) < TOL
    assert max(e_split) < TOL
    assert max(e_acc) < TOL
    assert torch.equal(dw, dw2) and torch.equal(db, db2)
