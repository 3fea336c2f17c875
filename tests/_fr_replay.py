"""Replay of every op call of one FrameRecoveryNet training step in float64, each on its own stored operands.

FrameRecoveryNet's step is an inner autograd graph of self-contained `nerve_cl._ops` Functions, so nothing in the library has to
be hooked: `Tape` wraps `.apply` of every `torch.autograd.Function` subclass of a namespace and records, per call, the arguments,
the output, the buffers the forward mutates, `ctx.saved_tensors`, the node's own (cloned) grad_outputs / grad_inputs and, for
the ops that write to an `InputGradSink`, the sink before and after the node ran.

`PLANS[op](args)` describes one op call: which arguments are differentiable tensors and how they are laid out (`Lay`), the
layout of the output, and `f(vals, q, aux)`: the op in plain torch, float64, NCHW, on the decoded operands.  The backward
replay is `torch.autograd.grad` of that same `f` for the recorded grad_outputs.  A replay never sees another replay's result.
The same plans serve two users:

  * `Checker` compares every stored tensor of a taped HIP run with its replay (the GPU tests, and the seeded defects of the
    CPU test);
  * `mirror_ops()` turns every plan into a float64 `torch.autograd.Function` with the op's signature and storage layout
    (channel padding included); `mirror_step` chains them in the network's op order into a whole training step, which
    tests/test_fr_replay_cpu.py holds against oracle/fr_oracle.py.  Taped, that step is the clean "stored" state the seeded
    defects are planted in.

Operand rounding.  `q` is `bf16_round` for an op called with MATH_BF16 and the identity otherwise.  The MFMA convolutions
(Conv, TemporalConv, SpatialConvTC, TemporalConvTC, ConvT) round the weights always and an fp32-stored activation or gradient
too (csrc/conv_common.h cvt4 / cvt8); the bias gradient sums the stored dy, not the rounded one (`_sr_replay.conv_wgrad`).
Stem7, DwConv, BatchNorm, pooling, CBAM, fusion, tanh and blend compute in fp32 on the stored values; the input gradient of
the first temporal conv (nvq_head_dgrad / nvq_head_dgrad_tc) is an fp32 kernel on the unrounded dy and weights.

Bounds are `_sr_replay.bound(kind, bf16_math, n_inner, grad)`; n_inner, the bf16 roundings inside an op beyond the stored
result's own, is written beside the plan that has any:
  * TemporalConv, bf16 storage, T > 1: the two shifted passes accumulate into the stored tensor, which is read back and rounded
    again each time (nerve_cl/_ops.py TemporalConv.forward / .backward, the `accumulate=True` launches; conv_common.h
    d.accumulate): 2, for y and for dx.
  * ConvT stores the phase-packed u (nerve_cl/_ops.py ConvT.forward, `u = _new(...)`) and nvq_depth_space2 copies it: the
    copy does not round again, 0.
  * MaxPool backward with overlapping windows (k > s): up to four window gradients per input pixel are summed in fp32 and
    rounded once (csrc/fr_ops.hip maxpool_bwd_kernel): 0, but not a copy - the stored kind's bound; disjoint windows copy.
  * everything else: one launch, one stored rounding, 0.
Conv's ReLU mask in the backward is the one of the stored y (nerve_cl/_ops.py Conv.backward), so no element is undecided.

Left out of a comparison (conditions on the float64 values, at most NEAR_CAP of a tensor, a larger share FAILS):
  * BatchNorm with relu, backward: the kernel decides pre > 0 in fp32 from the stored x, mean, invstd, gamma, beta, res
    (csrc/fr_ops.hip bn2_partial_kernel / bn2_bwd_apply_kernel).  Where the float64 |pre| < RELU_MARGIN * (|gamma*(x-mean)*invstd|
    + |beta| + |res|) the element is left out of dx and dres; in the sums behind dgamma, dbeta and dx the replay takes the
    decision the stored y shows for it.
  * CBAM's channel max: pixels whose two largest float64 values differ by less than RELU_MARGIN * (|a| + |b|) are left out of
    the amax comparison (the backward replays with the stored amax).
"""
from __future__ import annotations

import re
import types

import torch
import torch.nn.functional as F

from _sr_replay import NEAR_CAP, TOL_BF16, TOL_F32_FWD, TOL_F32_GRAD, TOL_F64, bf16_round, bound, ident  # noqa: F401

MATH_F32, MATH_BF16 = 0, 1              # nerve_cl._nvq's values (the GPU test asserts them)
BN_EPS, BN_MOMENTUM = 1e-5, 0.1
RELU_MARGIN = 1e-5                      # about 100 fp32 ulps of the summed terms
SINK_NAMES = ("dframe", "drefs", "dmask")

# the geometries of tests/test_fr_replay_gpu.py, the smallest that still reach every op form (frames of at least 32x32):
#  name, base, T, B,  H,  W, MATH_BF16, bf16 activations, time-in-channels, train, frozen
CASES = [
    ("A", 64, 4, 2, 64, 96, True, True, True, True, False),      # the bench's setting
    ("B", 64, 4, 2, 64, 96, True, True, False, True, False),     # time-major
    ("C", 64, 4, 2, 64, 96, True, False, True, True, False),     # fp32 activations (bf16 operands only)
    ("D", 64, 4, 2, 64, 96, True, True, True, False, False),     # eval: running statistics, BatchNorm backward in eval
    ("E", 32, 3, 1, 40, 72, True, True, True, True, False),      # Resize before the fusion and after the decoder, odd T
    ("F", 16, 1, 3, 33, 47, True, True, True, True, False),      # T = 1 takes the time-major path; odd sizes; 8-channel tail
    ("G", 64, 4, 2, 40, 72, False, False, True, True, False),    # MATH_F32, time-in-channels
    ("H", 16, 2, 2, 33, 47, False, False, False, True, False),   # MATH_F32, time-major
    ("I", 64, 4, 2, 64, 96, True, True, True, True, True),       # both encoders and one BatchNorm affine frozen
]


# ----------------------------------------------------------------------------- storage layouts
def layout_kind(t) -> str:
    """'bf16' or 'fp32': which padding rule a tensor follows (a mirror tensor is float64 and carries the kind it stands for)"""
    k = getattr(t, "_kind", None)
    return k or ("bf16" if t.dtype == torch.bfloat16 else "fp32")


def store_kind(t) -> str:
    """the storage precision a bound is chosen by"""
    return {torch.float64: "f64", torch.bfloat16: "bf16"}.get(t.dtype, "fp32")


def dk(dtype) -> str:
    return "bf16" if dtype == torch.bfloat16 else "fp32"


def padc(c: int, kind: str) -> int:
    return (c + 7) // 8 * 8 if kind == "bf16" else (c + 3) // 4 * 4


def tag(t, kind):
    t._kind = kind
    return t


class Lay:
    """[N,H,W,T*ld] with C real channels per frame; T > 1: time-in-channels, decoded as [N,T,C,H,W]"""

    def __init__(self, C, ld, T=1, kind="fp32"):
        self.C, self.ld, self.T, self.kind = C, ld, T, kind


def lay_of(t, C=None, T=1):
    ld = t.shape[-1] // T
    return Lay(ld if C is None else C, ld, T, layout_kind(t))


def dec(t, lay):
    """stored tensor -> float64 NCHW ([N,T,C,H,W] for a time-in-channels layout); lay None: as it is"""
    if lay is None:
        return t.detach().to(torch.float64)
    N, H, W, _ = t.shape
    v = t.detach().reshape(N, H, W, lay.T, lay.ld)[..., :lay.C].to(torch.float64).permute(0, 3, 4, 1, 2)
    return (v[:, 0] if lay.T == 1 else v).contiguous()


def pad_channels(t, lay):
    N, H, W, _ = t.shape
    return t.detach().reshape(N, H, W, lay.T, lay.ld)[..., lay.C:]


def enc(v, lay):
    """inverse of dec for the mirror: float64, zero padding channels, tagged with the storage kind it stands for"""
    if lay is None:
        return v.detach().clone()
    if lay.T == 1:
        v = v[:, None]
    N, T, C, H, W = v.shape
    out = torch.zeros(N, H, W, T, lay.ld, dtype=torch.float64, device=v.device)
    out[..., :C] = v.detach().permute(0, 3, 4, 1, 2)
    return tag(out.view(N, H, W, T * lay.ld), lay.kind)


def qs(q, t):
    """q(t) with the gradient of the identity: the kernel rounds the operand it reads, the gradient it writes is not rounded
    again on the way back (a cast inside the graph would round it)"""
    return t + (q(t.detach()) - t.detach())


class _QGrad(torch.autograd.Function):
    """identity whose gradient is rounded by q: the matrix-core kernels round an fp32-stored dy on its way into the MFMAs"""

    @staticmethod
    def forward(ctx, x, q):
        ctx.q = q
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        return ctx.q(g), None


def _args(a, n):
    return (list(a) + [None] * n)[:n]


class Plan:
    def __init__(self, ins, out, f, math=MATH_F32, n_out=0, n_in=None, exact=False, no_grad=(), aux=None, extra=None, sink=None,
                 mirror_fwd=None, skip=None, exact_grad=None):
        self.ins, self.out, self.f, self.math = ins, out, f, math
        self.n_out, self.n_in, self.exact, self.no_grad = n_out, n_in or {}, exact, set(no_grad)
        self.exact_grad = exact if exact_grad is None else exact_grad
        self.aux, self.extra, self.sink, self.mirror_fwd, self.skip = aux, extra, sink, mirror_fwd, skip


# ----------------------------------------------------------------------------- the ops in plain torch
def plan_Cast(a):
    x, dtype, C = a
    return Plan([(0, lay_of(x, C))], Lay(C, padc(C, dk(dtype)) if dk(dtype) != layout_kind(x) else x.shape[-1], 1, dk(dtype)),
                lambda v, q, aux: v[0] * 1.0)


def plan_Conv(a):
    x, w, b, relu, math, od, sink = _args(a, 7)
    Co, Ci, k, _ = w.shape
    okind = dk(od) if od is not None else layout_kind(x)
    sink = sink if sink is not None and sink.drefs is not None else None
    ins = [(0, lay_of(x, Ci)), (1, None)] + ([(2, None)] if b is not None else [])

    def f(v, q, aux):
        y = _QGrad.apply(F.conv2d(qs(q, v[0]), qs(q, v[1]), None, padding=k // 2), q)
        if b is not None:
            y = y + v[2].view(1, -1, 1, 1)
        if not relu:
            return y
        # backward: the mask is the one of the stored y (nvq_axpy_slice with mask = y)
        return y * aux["mask"] if aux and "mask" in aux else F.relu(y)

    def aux(e):
        return None, ({"mask": (dec(e["out"], Lay(Co, e["out"].shape[-1])) > 0).to(torch.float64)} if relu else None)

    def sink_fn(args, v, g, grads):
        # nvq_head_dgrad: fp32, unrounded dy and weights; time-major images [T*B] -> (B,T,3,H,W)
        assert not relu
        B, T = sink.drefs.shape[:2]
        dx = F.conv_transpose2d(g, v[1].detach(), None, padding=k // 2)
        return [("drefs", dx.view(T, B, *dx.shape[1:]).transpose(0, 1), "set")]

    return Plan(ins, Lay(Co, padc(Co, okind), 1, okind), f, math, aux=aux, no_grad=(0,) if sink else (),
                sink=sink_fn if sink else None)


def plan_DwConv(a):
    x, w = a
    C = w.shape[0]
    return Plan([(0, lay_of(x, C)), (1, None)], lay_of(x, C), lambda v, q, aux: F.conv2d(v[0], v[1], None, padding=1, groups=C))


def _temporal(xq, wq):
    """xq [T,B,Ci,H,W] -> [T,B,Co,H,W]: W1 x[t] + W0 x[t-1] + W2 x[t+1], zero padding in time"""
    w0, w1, w2 = (wq[:, :, k, 0, 0] for k in range(3))
    z = torch.zeros_like(xq[:1])
    y = torch.einsum("oi,tbihw->tbohw", w1, xq)
    y = y + torch.einsum("oi,tbihw->tbohw", w0, torch.cat([z, xq[:-1]], 0))
    return y + torch.einsum("oi,tbihw->tbohw", w2, torch.cat([xq[1:], z], 0))


def plan_TemporalConv(a):
    x, w, T, math = a
    Co, Ci = w.shape[:2]
    kind = layout_kind(x)

    def f(v, q, aux):
        xq = qs(q, v[0])
        y = _temporal(xq.view(T, xq.shape[0] // T, *xq.shape[1:]), qs(q, v[1]))
        return _QGrad.apply(y.reshape(xq.shape[0], Co, *xq.shape[2:]), q)

    # bf16 storage: the passes over x[t-1] and x[t+1] accumulate into the stored y / dx, re-rounded each time (see the module
    # docstring): two inner roundings
    n = 2 if (T > 1 and kind == "bf16") else 0
    return Plan([(0, lay_of(x, Ci)), (1, None)], Lay(Co, padc(Co, kind), 1, kind), f, math, n_out=n, n_in={0: n})


def plan_SpatialConvTC(a):
    x, w, T, math, od, sink = _args(a, 6)
    Co, Ci = w.shape[:2]
    okind = dk(od) if od is not None else layout_kind(x)
    sink = sink if sink is not None and sink.drefs is not None else None

    def f(v, q, aux):
        xq = qs(q, v[0])
        B = xq.shape[0]
        y = F.conv2d(xq.reshape(B * T, *xq.shape[2:]), qs(q, v[1]), None, padding=1)
        return _QGrad.apply(y.view(B, T, *y.shape[1:]), q)

    def sink_fn(args, v, g, grads):
        # nvq_head_dgrad_tc: fp32, unrounded dy and weights
        B = g.shape[0]
        dx = F.conv_transpose2d(g.reshape(B * T, *g.shape[2:]), v[1].detach(), None, padding=1)
        return [("drefs", dx.view(B, T, *dx.shape[1:]), "set")]

    return Plan([(0, lay_of(x, Ci, T)), (1, None)], Lay(Co, padc(Co, okind), T, okind), f, math, no_grad=(0,) if sink else (),
                sink=sink_fn if sink else None)


def plan_TemporalConvTC(a):
    x, w, T, math = a
    Co, Ci = w.shape[:2]
    kind = layout_kind(x)

    def f(v, q, aux):
        return _QGrad.apply(_temporal(qs(q, v[0]).transpose(0, 1), qs(q, v[1])).transpose(0, 1), q)

    return Plan([(0, lay_of(x, Ci, T)), (1, None)], Lay(Co, padc(Co, kind), T, kind), f, math)


def plan_GroupMean(a):
    x, T, C = a
    return Plan([(0, lay_of(x, C))], Lay(C, padc(C, "fp32"), 1, "fp32"),
                lambda v, q, aux: v[0].view(T, v[0].shape[0] // T, *v[0].shape[1:]).mean(0))


def plan_GroupMeanTC(a):
    x, T, C = a
    return Plan([(0, lay_of(x, C, T))], Lay(C, padc(C, "fp32"), 1, "fp32"), lambda v, q, aux: v[0].mean(1))


def plan_ConvT(a):
    x, w, math = a
    Ci, Co = w.shape[:2]
    kind = layout_kind(x)
    return Plan([(0, lay_of(x, Ci)), (1, None)], Lay(Co, Co, 1, kind),
                lambda v, q, aux: _QGrad.apply(F.conv_transpose2d(qs(q, v[0]), qs(q, v[1]), None, stride=2, padding=1), q), math)


def plan_Stem7(a):
    x4, w, od, sink = _args(a, 4)
    Co = w.shape[0]
    sink = sink if sink is not None and (sink.dframe is not None or sink.dmask is not None) else None

    def sink_fn(args, v, g, grads):
        # nvq_stem7_dgrad(accumulate=True): added to what MaskBlend wrote
        dx4 = grads[0]
        return [(n, d, "add") for n, d in (("dframe", dx4[:, :3]), ("dmask", dx4[:, 3:4])) if getattr(sink, n) is not None]

    return Plan([(0, lay_of(x4, 4)), (1, None)], Lay(Co, Co, 1, dk(od) if od is not None else "fp32"),
                lambda v, q, aux: F.conv2d(v[0], v[1], None, stride=2, padding=3), no_grad=(0,), sink=sink_fn if sink else None)


def plan_BatchNorm(a):
    x, gamma, beta, res, rmean, rvar, training, relu = a
    C = gamma.numel()
    lx = lay_of(x, C)
    ins = [(0, lx), (1, None), (2, None)] + ([(3, lay_of(res, C))] if res is not None else [])
    sh = (1, -1, 1, 1)
    run = (rmean.detach().to(torch.float64).clone(), rvar.detach().to(torch.float64).clone())

    def stats(xv):
        if training:
            return xv.mean(dim=(0, 2, 3)), torch.rsqrt(xv.var(dim=(0, 2, 3), unbiased=False) + BN_EPS)
        return run[0], torch.rsqrt(run[1] + BN_EPS)

    def pre_of(v, mean, inv):
        pre = (v[0] - mean.view(sh)) * (inv * v[1]).view(sh) + v[2].view(sh)
        return pre + v[3] if res is not None else pre

    def f(v, q, aux):
        mean, inv = (aux["mean"], aux["invstd"]) if aux and "mean" in aux else stats(v[0])
        pre = pre_of(v, mean, inv)
        if not relu:
            return pre
        return pre * aux["mask"] if aux and "mask" in aux else F.relu(pre)

    def aux(e):
        mean, inv = dec(e["saved"][4], None), dec(e["saved"][5], None)
        fwd = {"mean": mean, "invstd": inv}               # nvq_bn2_apply reads the stored statistics
        if not relu or "grad_outputs" not in e:
            return fwd, None
        v = [dec(e["args"][p], lay) for p, lay in ins]
        pre = pre_of(v, mean, inv)
        terms = ((v[0] - mean.view(sh)) * (inv * v[1]).view(sh)).abs() + v[2].abs().view(sh)
        if res is not None:
            terms = terms + v[3].abs()
        near = pre.abs() < RELU_MARGIN * terms
        mask = torch.where(near, dec(e["out"], lx) > 0, pre > 0).to(torch.float64)
        return fwd, {"mask": mask, "near": near}

    def skip(e, aux_b):
        return {0: aux_b["near"], 3: aux_b["near"]} if aux_b else {}

    def extra(e, v, emit):
        mean, inv = stats(v[0])
        emit(e, "mean", mean, dec(e["saved"][4], None), store_kind(e["saved"][4]))
        emit(e, "invstd", inv, dec(e["saved"][5], None), store_kind(e["saved"][5]))
        if training:
            n = v[0].numel() // C
            var = v[0].var(dim=(0, 2, 3), unbiased=False) * (n / max(n - 1, 1))
            b0, b1 = e["buf_before"], e["buf_after"]
            emit(e, "running_mean", (1 - BN_MOMENTUM) * dec(b0[0], None) + BN_MOMENTUM * mean, dec(b1[0], None), store_kind(b1[0]))
            emit(e, "running_var", (1 - BN_MOMENTUM) * dec(b0[1], None) + BN_MOMENTUM * var, dec(b1[1], None), store_kind(b1[1]))

    def mirror_fwd(args, v, y):
        mean, inv = stats(v[0].detach())
        if training:
            n = v[0].numel() // C
            var = v[0].detach().var(dim=(0, 2, 3), unbiased=False) * (n / max(n - 1, 1))
            with torch.no_grad():
                rmean.mul_(1 - BN_MOMENTUM).add_(BN_MOMENTUM * mean)
                rvar.mul_(1 - BN_MOMENTUM).add_(BN_MOMENTUM * var)
        return (None, None, None, None, mean.clone(), inv.clone())

    return Plan(ins, lx, f, aux=aux, extra=extra, mirror_fwd=mirror_fwd, skip=skip)


def _window_index(xv, k, s, pad):
    """ky * k + kx of the first maximum in (ky, kx) scan order (csrc/fr_ops.hip maxpool_fwd_kernel)"""
    W = xv.shape[-1]
    _, ind = F.max_pool2d(xv, k, s, pad, return_indices=True)
    oy = torch.arange(ind.shape[-2], device=xv.device).view(-1, 1)
    ox = torch.arange(ind.shape[-1], device=xv.device).view(1, -1)
    return (torch.div(ind, W, rounding_mode="floor") - (oy * s - pad)) * k + (ind % W - (ox * s - pad))


def plan_MaxPool(a):
    x, k, s, pad = a
    lx = lay_of(x)

    def extra(e, v, emit):
        emit(e, "idx", _window_index(v[0], k, s, pad).to(torch.float64), dec(e["saved"][0], lx), "int", exact=True)

    # overlapping windows (k > s): an input pixel collects up to four window gradients, summed in fp32 and rounded once
    # (maxpool_bwd_kernel's gather form): the stored kind's bound; disjoint windows copy
    return Plan([(0, lx)], lx, lambda v, q, aux: F.max_pool2d(v[0], k, s, pad), exact=True, exact_grad=k <= s, extra=extra,
                mirror_fwd=lambda args, v, y: (enc(_window_index(v[0].detach(), k, s, pad).to(torch.float64), lx),))


def plan_Subsample2(a):
    lx = lay_of(a[0])
    return Plan([(0, lx)], lx, lambda v, q, aux: v[0][:, :, ::2, ::2], exact=True)


def plan_Resize(a):
    x, OH, OW = a
    lx = lay_of(x)
    return Plan([(0, lx)], lx, lambda v, q, aux: F.interpolate(v[0], size=(OH, OW), mode="bilinear", align_corners=False))


def plan_Cat2(a):
    x, y = a
    return Plan([(0, lay_of(x)), (1, lay_of(y))], Lay(x.shape[-1] + y.shape[-1], x.shape[-1] + y.shape[-1]),
                lambda v, q, aux: torch.cat([v[0], v[1]], 1), exact=True)


def plan_DepthToSpace2(a):
    u, = a
    Co = u.shape[-1] // 4

    def f(v, q, aux):
        N, _, H, W = v[0].shape
        return v[0].view(N, 2, 2, Co, H, W).permute(0, 3, 4, 1, 5, 2).reshape(N, Co, 2 * H, 2 * W)

    return Plan([(0, lay_of(u))], Lay(Co, Co, 1, layout_kind(u)), f, exact=True)


def cbam_parts(x, w1, w2, w7, amax=None, gap=None, hid=None, ca=None, sm=None):
    """CBAM stage by stage; a stage given as an argument is taken as stored instead of computed"""
    p = {}
    p["gap"] = x.mean(dim=(2, 3))
    p["hid"] = F.relu((p["gap"] if gap is None else gap) @ w1.t())
    p["ca"] = torch.sigmoid((p["hid"] if hid is None else hid) @ w2.t())
    xc = x * (p["ca"] if ca is None else ca)[:, :, None, None]
    mx = xc.max(dim=1)[0]
    p["amax"] = (xc == mx[:, None]).to(torch.float64).argmax(dim=1)          # ties go to the first maximum
    top = xc.detach().topk(2, dim=1)[0]
    p["near"] = (top[:, 0] - top[:, 1]) < RELU_MARGIN * (top[:, 0].abs() + top[:, 1].abs())
    if amax is not None:
        mx = xc.gather(1, amax[:, None])[:, 0]
    p["sm"] = torch.stack([xc.mean(dim=1), mx], 1)
    p["sa"] = torch.sigmoid(F.conv2d(p["sm"] if sm is None else sm, w7, None, padding=3))[:, 0]
    p["y"] = xc * p["sa"][:, None]
    return p


def plan_CBAMFn(a):
    x = a[0]
    lx = lay_of(x)
    sm_lay = Lay(2, 2)

    def f(v, q, aux):
        return cbam_parts(*v, amax=aux["amax"] if aux else None)["y"]

    def aux(e):
        return None, {"amax": e["saved"][8].detach().long()}

    def extra(e, v, emit):
        s = e["saved"]
        gap, hid, ca, sm = dec(s[4], None), dec(s[5], None), dec(s[6], None), dec(s[7], sm_lay)
        p = cbam_parts(*v, gap=gap, hid=hid, ca=ca, sm=sm)
        emit(e, "gap", p["gap"], gap, store_kind(s[4]))
        emit(e, "hid", p["hid"], hid, store_kind(s[5]))
        emit(e, "ca", p["ca"], ca, store_kind(s[6]))
        emit(e, "sm", p["sm"], sm, store_kind(s[7]))
        emit(e, "amax", p["amax"].to(torch.float64), dec(s[8], None), "int", exact=True, skip=p["near"])
        emit(e, "sa", p["sa"], dec(s[9], None), store_kind(s[9]))

    def mirror_fwd(args, v, y):
        p = cbam_parts(*[t.detach() for t in v])
        return (None, None, None, None, p["gap"], p["hid"], p["ca"], enc(p["sm"], sm_lay), p["amax"].to(torch.float64), p["sa"])

    return Plan([(0, lx), (1, None), (2, None), (3, None)], lx, f, aux=aux, extra=extra, mirror_fwd=mirror_fwd)


def plan_FusionMix(a):
    al, lg, sp, tp = a

    def f(v, q, aux):
        at = torch.softmax(v[1], dim=1)
        return v[0] + at[:, 0:1] * v[2].mean(1, keepdim=True) + at[:, 1:2] * v[3].mean(1, keepdim=True)

    def parts(v):
        at = torch.softmax(v[1], dim=1).permute(0, 2, 3, 1).reshape(-1, 2)
        return at, torch.stack([v[2].mean(1), v[3].mean(1)], -1).reshape(-1, 2)

    def extra(e, v, emit):
        # what the backward reads: the softmax weights and the two channel means per pixel (nvq_fusion_mix_forward)
        at, means = parts(v)
        emit(e, "attn", at, dec(e["saved"][0], None), store_kind(e["saved"][0]))
        emit(e, "means", means, dec(e["saved"][1], None), store_kind(e["saved"][1]))

    return Plan([(0, lay_of(al)), (1, lay_of(lg, 2)), (2, lay_of(sp)), (3, lay_of(tp))], lay_of(al), f, extra=extra,
                mirror_fwd=lambda args, v, y: parts([t.detach() for t in v]))


def plan_Tanh(a):
    lx = lay_of(a[0])
    return Plan([(0, lx)], lx, lambda v, q, aux: torch.tanh(v[0]))


def plan_MaskBlend(a):
    frame, rec, mask, sink = _args(a, 4)
    C = frame.shape[1]
    sink = sink if sink is not None and (sink.dframe is not None or sink.dmask is not None) else None
    fr, mk = dec(frame, None), dec(mask, None)

    def sink_fn(args, v, g, grads):
        w = [("dframe", g * (1 - mk), "set"), ("dmask", (g * (v[0].detach() - fr)).sum(1, keepdim=True), "set")]
        return [t for t in w if getattr(sink, t[0]) is not None]

    return Plan([(1, lay_of(rec, C))], None, lambda v, q, aux: fr * (1 - mk) + v[0] * mk, sink=sink_fn if sink else None)


PLANS = {n[5:]: f for n, f in list(globals().items()) if n.startswith("plan_")}


# ----------------------------------------------------------------------------- the tape
def _find_sink(args):
    for x in args:
        if x is not None and not isinstance(x, torch.Tensor) and all(hasattr(x, n) for n in SINK_NAMES):
            return x
    return None


def _snap(sink):
    return {n: getattr(sink, n).detach().clone() for n in SINK_NAMES if getattr(sink, n) is not None}


class Tape:
    """Context manager: records every call of `Cls.apply` for each torch.autograd.Function subclass found in `ns` (a module or
    a namespace).  entries[i]: op, idx, args, out, grad_mode, and when the output has a grad_fn: saved, needs, and after the
    backward grad_outputs / grad_inputs (clones), bwd_order, sink_before / sink_after."""

    def __init__(self, ns):
        self.ns, self.entries, self._orig, self._bwd = ns, [], {}, 0
        self.classes = {n: c for n, c in vars(ns).items()
                        if isinstance(c, type) and issubclass(c, torch.autograd.Function) and c is not torch.autograd.Function}

    def __enter__(self):
        for name, cls in self.classes.items():
            self._orig[name] = ("apply" in cls.__dict__, cls.__dict__.get("apply"))
            cls.apply = staticmethod(self._recorder(name, cls.apply))
        return self

    def __exit__(self, *exc):
        for name, cls in self.classes.items():
            had, old = self._orig[name]
            if had:
                setattr(cls, "apply", old)
            else:
                delattr(cls, "apply")
        return False

    def _recorder(self, name, orig):
        def rec(*args):
            e = {"op": name, "idx": len(self.entries), "args": args, "grad_mode": torch.is_grad_enabled()}
            self.entries.append(e)
            if name == "BatchNorm":
                e["buf_before"] = (args[4].detach().clone(), args[5].detach().clone())
            out = orig(*args)
            e["out"] = out
            if name == "BatchNorm":
                e["buf_after"] = (args[4].detach().clone(), args[5].detach().clone())
            fn = out.grad_fn if isinstance(out, torch.Tensor) and torch.is_grad_enabled() else None
            if fn is None:
                return out
            e["saved"] = tuple(getattr(fn, "saved_tensors", ()))
            e["needs"] = tuple(fn.needs_input_grad)

            def hook(grad_inputs, grad_outputs):
                e["grad_inputs"] = [None if g is None else g.detach().clone() for g in grad_inputs]
                e["grad_outputs"] = [None if g is None else g.detach().clone() for g in grad_outputs]
                e["bwd_order"] = self._bwd
                self._bwd += 1
                if sink is not None:
                    e["sink_after"] = _snap(sink)

            sink = _find_sink(args)
            if sink is not None:
                fn.register_prehook(lambda grad_outputs: e.__setitem__("sink_before", _snap(sink)))
            fn.register_hook(hook)
            return out
        return rec


# ----------------------------------------------------------------------------- the checker
class Checker:
    """compares every stored tensor of a tape with its replay; rows: (launch, key, rel, rel_l2, bound, ok)"""

    def __init__(self, bf16_math: bool, names=None):
        """names: {data_ptr: parameter name} of the parameters whose gradients are to be claimed"""
        self.bf16_math, self.names = bf16_math, names or {}
        self.rows, self.claimed, self.unknown, self.sink_writes, self.grads, self.shares = [], [], [], [], {}, {}

    def emit(self, e, key, want, got, kind, n_inner=0, grad=False, exact=False, skip=None):
        launch = f"{e['op']}[{e['idx']}]"
        assert got.shape == want.shape, (launch, key, tuple(got.shape), tuple(want.shape))
        got, want = got.to(torch.float64), want.detach().to(torch.float64)
        keep = None
        if skip is not None:
            share = skip.to(torch.float64).mean().item()
            self.shares[(launch, key)] = share
            if share > NEAR_CAP:                    # too many elements left out: a failure, not a skip
                self.rows.append((launch, key + " (left out)", share, share, NEAR_CAP, False))
                return
            keep = ~skip
            keep = keep[:, None].expand_as(want) if keep.dim() == want.dim() - 1 else keep
        if exact:
            bad = got != want
            if keep is not None:
                bad = bad & keep
            nbad = int(bad.sum())
            self.rows.append((launch, key, float(nbad), float(nbad), 0.0, nbad == 0))
            return
        d = got - want
        if keep is not None:
            d, want = d * keep, want * keep
        scale = want.abs().max().clamp_min(1e-300)
        rel = (d.abs().max() / scale).item()
        l2 = (d.norm() / want.norm().clamp_min(1e-300)).item()
        b = bound(kind, self.bf16_math, n_inner, grad)
        self.rows.append((launch, key, rel, l2, b, rel <= b))

    def _pad(self, e, key, t, lay):
        if lay is not None and lay.ld > lay.C:
            p = pad_channels(t, lay).to(torch.float64)
            self.emit(e, "pad:" + key, torch.zeros_like(p), p, "int", exact=True)

    def check(self, entries):
        for e in entries:
            if e["op"] not in PLANS:
                self.unknown.append(e["op"])
                continue
            self.check_entry(e)
        return self

    def check_entry(self, e):
        a = e["args"]
        plan = PLANS[e["op"]](a)
        q = bf16_round if (plan.math == MATH_BF16 and self.bf16_math) else ident
        vals = [dec(a[p], lay) for p, lay in plan.ins]
        aux_f, aux_b = plan.aux(e) if (plan.aux and "saved" in e) else (None, None)
        out = e["out"]
        self.emit(e, "out", plan.f(vals, q, aux_f), dec(out, plan.out), store_kind(out), n_inner=plan.n_out, exact=plan.exact)
        self._pad(e, "out", out, plan.out)
        if plan.extra and "saved" in e:
            plan.extra(e, vals, self.emit)
        if "grad_outputs" not in e:
            return
        tpos = [i for i, t in enumerate(a) if isinstance(t, torch.Tensor)]
        gin = e["grad_inputs"]
        assert len(gin) == len(tpos), (e["op"], len(gin), len(tpos))
        leaves = [v.clone().requires_grad_() for v in vals]
        g = dec(e["grad_outputs"][0], plan.out)
        grads = torch.autograd.grad(plan.f(leaves, q, aux_b), leaves, g, allow_unused=True)
        skips = plan.skip(e, aux_b) if plan.skip else {}
        for (p, lay), want in zip(plan.ins, grads):
            got = gin[tpos.index(p)]
            name = self.names.get(a[p].data_ptr())
            key = f"grad:{name}" if name else f"d.arg{p}"
            if got is None or p in plan.no_grad:
                # no gradient launch: only where none was asked for (a frozen parameter, an input that goes to the sink)
                ok = got is None and (p in plan.no_grad or not e["needs"][p])
                if not ok:
                    self.rows.append((f"{e['op']}[{e['idx']}]", key + " (missing or unexpected)", 1.0, 1.0, 0.0, False))
                continue
            if name:
                self.claimed.append(name)
                self.grads[name] = got
            self.emit(e, key, want if want is not None else torch.zeros_like(vals[0]), dec(got, lay), store_kind(got),
                      n_inner=plan.n_in.get(p, 0), grad=True, exact=plan.exact_grad, skip=skips.get(p))
            self._pad(e, key, got, lay)
        if plan.sink:
            by_pos = {p: gr for (p, _), gr in zip(plan.ins, grads)}
            for name, val, mode in plan.sink(a, vals, g, by_pos):
                before, after = e["sink_before"][name], e["sink_after"][name]
                want = val + dec(before, None) if mode == "add" else val
                self.emit(e, "sink." + name, want, dec(after, None), store_kind(after), grad=True)
                self.sink_writes.append((e["bwd_order"], name, mode, before, after))

    def input_accounting(self, final):
        """final: {dframe, drefs, dmask: the network's input gradient}.  Each must be what the sink-writing ops left: the first
        writer sets it, every later one adds to exactly what the one before left, and the last state is the delivered
        gradient.  Returns the list of complaints."""
        bad = []
        for name in SINK_NAMES:
            w = sorted((x for x in self.sink_writes if x[1] == name), key=lambda x: x[0])
            if final.get(name) is None:
                continue
            if not w:
                bad.append(f"{name}: no taped op writes it")
                continue
            if w[0][2] != "set":
                bad.append(f"{name}: its first writer accumulates into an unset buffer")
            for prev, cur in zip(w, w[1:]):
                if cur[2] != "add" or not torch.equal(prev[4], cur[3]):
                    bad.append(f"{name}: a write between two taped writers")
            if not torch.equal(w[-1][4], final[name].detach().to(w[-1][4].dtype)):
                bad.append(f"{name}: the delivered gradient is not what the last writer left")
        return bad

    def failures(self):
        return [r for r in self.rows if not r[5]]

    def report(self):
        return "\n".join(f"  {'ok  ' if ok else 'FAIL'} {launch:22s} {key:60s} rel {rel:.2e}  l2 {l2:.2e}  bound {b:.1e}"
                         for launch, key, rel, l2, b, ok in self.rows)

    def worst_by_class(self):
        """{(op class, bound class): worst rel}"""
        out = {}
        for launch, key, rel, l2, b, ok in self.rows:
            cls = re.sub(r"\[\d+\]", "", launch)
            kind = "exact" if b == 0.0 else f"{b:.1e}"
            out[(cls, kind)] = max(out.get((cls, kind), 0.0), rel)
        return out


# ----------------------------------------------------------------------------- the float64 mirror
def _mirror_class(name):
    def forward(ctx, *args):
        plan = PLANS[name](args)
        vals = [dec(args[p], lay).requires_grad_(True) for p, lay in plan.ins]
        with torch.enable_grad():
            y = plan.f(vals, ident, None)
        ctx.state = (plan, vals, y, args)
        if plan.mirror_fwd:
            ctx.save_for_backward(*plan.mirror_fwd(args, vals, y))
        return enc(y, plan.out)

    def backward(ctx, dy):
        plan, vals, y, args = ctx.state
        g = dec(dy, plan.out)
        grads = torch.autograd.grad(y, vals, g, allow_unused=True)
        res = [None] * len(args)
        for (p, lay), gr in zip(plan.ins, grads):
            if p not in plan.no_grad and ctx.needs_input_grad[p] and gr is not None:
                res[p] = enc(gr, lay)
        if plan.sink:
            sink = _find_sink(args)
            for nm, val, mode in plan.sink(args, vals, g, {p: gr for (p, _), gr in zip(plan.ins, grads)}):
                t = getattr(sink, nm)
                t.copy_(t + val if mode == "add" else val)
        return tuple(res)

    return type(name, (torch.autograd.Function,), {"forward": staticmethod(forward), "backward": staticmethod(backward)})


def mirror_ops():
    """a namespace with one float64 Function per plan, same name and positional signature as in nerve_cl._ops"""
    return types.SimpleNamespace(**{name: _mirror_class(name) for name in PLANS})


def _nhwc(img, ld, kind="fp32"):
    N, C, H, W = img.shape
    out = torch.zeros(N, H, W, ld, dtype=torch.float64)
    out[..., :C] = img.detach().permute(0, 2, 3, 1)
    return tag(out, kind)


def mirror_graph(M, P, frame, refs, mask, sink, training, tic, act):
    """FrameRecoveryNet._graph with the mirror ops: same calls, same order, same storage layouts.  P: {state_dict name: float64
    tensor} (the BatchNorm buffers are updated in place); act: torch.bfloat16 / torch.float32 (which layouts the encoders and
    the decoder use); returns the NCHW output and the list of input leaves."""
    B, C, H, W = frame.shape
    T = refs.shape[1]
    f32, math = torch.float32, MATH_F32
    leaves = []

    def bn(pre, x, relu, res=None):
        return M.BatchNorm.apply(x, P[pre + "weight"], P[pre + "bias"], res, P[pre + "running_mean"], P[pre + "running_var"],
                                 training, relu)

    def bn_tc(pre, x, relu):
        b, h, w, ld = x.shape
        v = tag(x.view(b, h, w * T, ld // T), layout_kind(x))
        return tag(bn(pre, v, relu).view(b, h, w, ld), layout_kind(x))

    def res_block(pre, x):
        y = M.DwConv.apply(x, P[pre + "conv1.depthwise.weight"])
        y = bn(pre + "conv1.bn.", M.Conv.apply(y, P[pre + "conv1.pointwise.weight"], None, False, math), True)
        y = M.DwConv.apply(y, P[pre + "conv2.0.weight"])
        return bn(pre + "conv2.2.", M.Conv.apply(y, P[pre + "conv2.1.weight"], None, False, math), True, res=x)

    def cbam(pre, x):
        return M.CBAMFn.apply(x, P[pre + "channel_attention.fc.0.weight"], P[pre + "channel_attention.fc.2.weight"],
                              P[pre + "spatial_attention.conv.weight"])

    x4 = _nhwc(torch.cat([frame, mask], 1), 4)
    if sink is not None and (sink.dframe is not None or sink.dmask is not None):
        leaves.append(x4.requires_grad_())
    se = "spatial_encoder."
    y = bn(se + "stem.1.", M.Stem7.apply(x4, P[se + "stem.0.weight"], act, sink), True)
    y = M.MaxPool.apply(y, 3, 2, 1)
    for si in (1, 2, 3):
        idx = 0
        if si > 1:
            y = M.Conv.apply(M.Subsample2.apply(y), P[f"{se}stage{si}.0.0.weight"], None, False, math)
            y = bn(f"{se}stage{si}.0.1.", y, False)
            idx = 1
        for b in range(2):
            y = res_block(f"{se}stage{si}.{idx + b}.", y)
    sp = cbam(se + "attention.", M.Cast.apply(y, f32, y.shape[-1]))

    te = "temporal_encoder."
    w3 = lambda n: P[n].view(P[n].shape[0], P[n].shape[1], 3, 3)          # noqa: E731
    if T >= 2 and tic:
        r = tag(torch.cat([_nhwc(refs[:, t], 4) for t in range(T)], -1), "fp32")
        if sink is not None and sink.drefs is not None:
            leaves.append(r.requires_grad_())
        y = r
        for i, name in enumerate(("conv1", "conv2", "conv3")):
            y = M.SpatialConvTC.apply(y, w3(f"{te}{name}.spatial.0.weight"), T, math, act if i == 0 else None, sink if i == 0 else None)
            y = bn_tc(f"{te}{name}.spatial.1.", y, True)
            y = bn_tc(f"{te}{name}.temporal.1.", M.TemporalConvTC.apply(y, P[f"{te}{name}.temporal.0.weight"], T, math), True)
            if i < 2:
                y = M.MaxPool.apply(y, 2, 2, 0)
        tp = M.GroupMeanTC.apply(y, T, P[te + "conv3.temporal.0.weight"].shape[0])
    else:
        r = tag(torch.cat([_nhwc(refs[:, t], 4) for t in range(T)], 0), "fp32")
        if sink is not None and sink.drefs is not None:
            leaves.append(r.requires_grad_())
        y = r
        for i, name in enumerate(("conv1", "conv2", "conv3")):
            y = M.Conv.apply(y, w3(f"{te}{name}.spatial.0.weight"), None, False, math, act if i == 0 else None, sink if i == 0 else None)
            y = bn(f"{te}{name}.spatial.1.", y, True)
            y = bn(f"{te}{name}.temporal.1.", M.TemporalConv.apply(y, P[f"{te}{name}.temporal.0.weight"], T, math), True)
            if i < 2:
                y = M.MaxPool.apply(y, 2, 2, 0)
        tp = M.GroupMean.apply(y, T, P[te + "conv3.temporal.0.weight"].shape[0])

    if sp.shape[1:3] != tp.shape[1:3]:
        tp = M.Resize.apply(tp, sp.shape[1], sp.shape[2])
    al = M.Conv.apply(M.Cat2.apply(sp, tp), P["fusion.align.weight"], P["fusion.align.bias"], False, math)
    at = M.Conv.apply(al, P["fusion.attention.0.weight"], P["fusion.attention.0.bias"], True, math)
    lg = M.Conv.apply(at, P["fusion.attention.2.weight"], P["fusion.attention.2.bias"], False, math)
    y = M.FusionMix.apply(al, lg, sp, tp)
    y = cbam("fusion.refine.2.", res_block("fusion.refine.1.", res_block("fusion.refine.0.", y)))

    x = M.Cast.apply(y, act, y.shape[-1])
    for i in (1, 2, 3, 4):
        x = bn(f"decoder.up{i}.1.", M.ConvT.apply(x, P[f"decoder.up{i}.0.weight"], math), True)
    rec = M.Tanh.apply(M.Conv.apply(x, P["decoder.final.0.weight"], P["decoder.final.0.bias"], False, math, f32))
    if rec.shape[1:3] != (H, W):
        rec = M.Resize.apply(rec, H, W)
    return M.MaskBlend.apply(frame, rec, mask, sink), leaves


def mirror_step(sd, frame, refs, mask, tgt, training, tic, act, tape=True):
    """one float64 training step of the mirror (MSE loss) -> dict(out, grads, sink, P, before, entries, M)"""
    P = {k: (v.detach().to(torch.float64).clone().requires_grad_("running" not in k) if v.is_floating_point() else v.clone())
         for k, v in sd.items()}
    before = {k: v.clone() for k, v in P.items() if "running" in k}
    frame, refs, mask = (t.to(torch.float64) for t in (frame, refs, mask))
    sink = types.SimpleNamespace(dframe=torch.zeros_like(frame), drefs=torch.zeros_like(refs), dmask=torch.zeros_like(mask))
    M = mirror_ops()
    names = [k for k, v in P.items() if v.is_floating_point() and v.requires_grad]
    with Tape(M) as tp:
        out, leaves = mirror_graph(M, P, frame, refs, mask, sink, training, tic, act)
        loss = F.mse_loss(out, tgt.to(torch.float64))
        grads = torch.autograd.grad(loss, [P[n] for n in names] + leaves, allow_unused=True)[:len(names)]
    return {"out": out.detach(), "grads": dict(zip(names, grads)), "sink": sink, "P": P, "entries": tp.entries,
            "bn": {k: P[k].detach() - v for k, v in before.items()}, "names": {P[n].data_ptr(): n for n in names}}
