"""CPU oracle for the reference's FrameRecoveryNet (BASELINE cfg4) - groundwork for the HIP
build of that network, which does not exist yet.

TEST INFRASTRUCTURE ONLY, like everything under ``oracle/``: nothing in the product imports it.

The forward pass of ``nerve_cl.models.frame_recovery.FrameRecoveryNet`` (reference ``nerve_cl/models/frame_recovery.py``
and the layers of ``nerve_cl/models/layers/efficient_layers.py`` it is built from) restated as plain functions over a flat
``{state_dict name: tensor}`` dictionary; autograd supplies the backward.  Each function cites the reference lines it follows.

Parity pin: ``oracle/make_goldens.py --only-fr`` imports the reference in the build container, drives it and this
restatement with the same formula-generated weights / inputs, asserts agreement and writes ``tests/golden/fr_*.npz``;
``tests/test_oracle_golden.py`` checks this file against those fixtures on every CPU run.

Precision modes (``prec``): None is the reference's arithmetic (float64 in, float64 out, no rounding).  "bf16_operands"
rounds what the HIP network's ``MATH_BF16`` mode hands its MFMA convolutions to bf16 and nothing else (FrameRecoveryNet with
``bf16_activations=False``); "bf16_storage" also rounds every tensor that mode stores as bf16, forward and backward
(``bf16_activations=True``, the default).  Rounding is float -> float32 -> bf16, round-to-nearest-even, as the kernels' ``(__bf16)``
casts (csrc/conv_common.h cvt4 / cvt8, csrc/common.h stx4).  Each rounding point below names the HIP op it mirrors.
"""
from __future__ import annotations

from typing import Dict, List, Tuple

import torch
import torch.nn.functional as F

Params = Dict[str, torch.Tensor]
BN_EPS, BN_MOMENTUM = 1e-5, 0.1        # nn.BatchNorm2d / BatchNorm3d defaults
PRECISIONS = (None, "bf16_operands", "bf16_storage")


# ---------------------------------------------------------------------------- bf16 emulation
def bf16_round(t: torch.Tensor) -> torch.Tensor:
    """t rounded to bf16 as the kernels' (__bf16) casts of fp32 values do (round to nearest, ties to even), in t's dtype"""
    return t.to(torch.float32).to(torch.bfloat16).to(t.dtype)


class _Bf16Conv(torch.autograd.Function):
    """fn(x, w) (F.conv2d / F.conv3d / F.conv_transpose2d, no bias) with the operands of MATH_BF16 rounded: the forward takes
    bf16(x) and bf16(w), the input gradient bf16(dy) and bf16(w), the weight gradient bf16(x) and bf16(dy); every sum is
    float64 (nerve_cl._ops Conv / TemporalConv / SpatialConvTC / TemporalConvTC / ConvT, conv_forward and conv_wgrad with
    math=MATH_BF16).  exact_dgrad: the input gradient is the fp32 kernel's, from the unrounded dy and w (nvq_head_dgrad /
    nvq_head_dgrad_tc: FrameRecoveryNet's first temporal conv)."""

    @staticmethod
    def forward(ctx, x, w, fn, kw, exact_dgrad):
        xr, wr = bf16_round(x), bf16_round(w)
        ctx.save_for_backward(xr, wr, w)
        ctx.fn, ctx.kw, ctx.exact_dgrad = fn, kw, exact_dgrad
        return fn(xr, wr, None, **kw)

    @staticmethod
    def backward(ctx, dy):
        xr, wr, w = ctx.saved_tensors
        fn, kw = ctx.fn, ctx.kw
        need_x, need_w = ctx.needs_input_grad[:2]
        dx = dw = None
        with torch.enable_grad():
            xa, wa = xr.detach().requires_grad_(), wr.detach().requires_grad_()
            if need_w or (need_x and not ctx.exact_dgrad):
                dx, dw = torch.autograd.grad(fn(xa, wa, None, **kw), (xa, wa), bf16_round(dy))
            if need_x and ctx.exact_dgrad:
                we = w.detach().requires_grad_()
                dx, = torch.autograd.grad(fn(xa, we, None, **kw), (xa,), dy)
        return (dx if need_x else None), (dw if need_w else None), None, None, None


class _Bf16Store(torch.autograd.Function):
    """a tensor that the HIP network stores as bf16: rounded on the way forward, its gradient (stored as bf16 too: every op's
    backward writes its input gradient in its input's storage type) rounded on the way back"""

    @staticmethod
    def forward(ctx, x):
        return bf16_round(x)

    @staticmethod
    def backward(ctx, dy):
        return bf16_round(dy)


class _Bf16GradOnly(torch.autograd.Function):
    """identity forward; the gradient rounded: one consumer's share of the gradient of a bf16-stored tensor with several
    consumers, rounded by that consumer's backward before autograd adds the shares (a bf16 add: rounded again at the tensor)"""

    @staticmethod
    def forward(ctx, x):
        return x.view_as(x)

    @staticmethod
    def backward(ctx, dy):
        return bf16_round(dy)


def conv(fn, x: torch.Tensor, w: torch.Tensor, b=None, prec=None, exact_dgrad: bool = False, **kw) -> torch.Tensor:
    """every convolution of the network that runs on the MFMA kernels: fn(x, w, b, **kw), with bf16 operands unless prec is None.
    The bias is fp32 in the kernels' epilogue and its gradient the sum of the unrounded dy (conv_bf16.hip wgrad_bf16_kernel
    bsumA / bsumB, wgrad_m32.hip bsum)."""
    if prec is None:
        return fn(x, w, b, **kw)
    y = _Bf16Conv.apply(x, w, fn, kw, exact_dgrad)
    if b is not None:
        y = y + b.view([1, -1] + [1] * (y.dim() - 2))
    return y


def store(x: torch.Tensor, prec) -> torch.Tensor:
    """a bf16 storage point (prec "bf16_storage"); the identity otherwise"""
    return _Bf16Store.apply(x) if prec == "bf16_storage" else x


def grad_share(x: torch.Tensor, prec) -> torch.Tensor:
    """one consumer's gradient share of a bf16-stored tensor (prec "bf16_storage"); the identity otherwise"""
    return _Bf16GradOnly.apply(x) if prec == "bf16_storage" else x


class _Bf16TemporalAccum(torch.autograd.Function):
    """Conv3d(Ci, Co, (3,1,1), padding (1,0,0)) as the time-major layout runs it with bf16 storage (nerve_cl._ops
    TemporalConv): three 1x1 convolutions over shifted frame ranges, each ACCUMULATING into the bf16 output (the conv
    epilogue reads the stored value, adds, rounds: conv_common.h d.accumulate).  Forward y[t] = r(r(r(W1 x[t]) + W0 x[t-1])
    + W2 x[t+1]); input gradient dx[t] = r(r(r(W1' g[t]) + W0' g[t+1]) + W2' g[t-1]) in the same launch order; the tap
    gradients are plain sums.  x (B, Ci, T, H, W); operands rounded as in _Bf16Conv."""

    @staticmethod
    def _taps(a, wk):
        return torch.einsum("oi,bithw->bothw", wk, a)

    @staticmethod
    def forward(ctx, x, w):
        xr, wr = bf16_round(x), bf16_round(w)
        ctx.save_for_backward(xr, wr)
        W0, W1, W2 = (wr[:, :, k, 0, 0] for k in range(3))
        y = bf16_round(_Bf16TemporalAccum._taps(xr, W1))
        y[:, :, 1:] = bf16_round(y[:, :, 1:] + _Bf16TemporalAccum._taps(xr[:, :, :-1], W0))
        y[:, :, :-1] = bf16_round(y[:, :, :-1] + _Bf16TemporalAccum._taps(xr[:, :, 1:], W2))
        return y

    @staticmethod
    def backward(ctx, dy):
        xr, wr = ctx.saved_tensors
        g = bf16_round(dy)
        W0, W1, W2 = (wr[:, :, k, 0, 0].t() for k in range(3))
        tap = _Bf16TemporalAccum._taps
        dx = bf16_round(tap(g, W1))
        dx[:, :, :-1] = bf16_round(dx[:, :, :-1] + tap(g[:, :, 1:], W0))
        dx[:, :, 1:] = bf16_round(dx[:, :, 1:] + tap(g[:, :, :-1], W2))
        dw = torch.zeros_like(wr)
        dw[:, :, 1, 0, 0] = torch.einsum("bothw,bithw->oi", g, xr)
        dw[:, :, 0, 0, 0] = torch.einsum("bothw,bithw->oi", g[:, :, 1:], xr[:, :, :-1])
        dw[:, :, 2, 0, 0] = torch.einsum("bothw,bithw->oi", g[:, :, :-1], xr[:, :, 1:])
        return dx, dw


# ---------------------------------------------------------------------------- parameter inventory
def _bn(shapes, buffers, pre: str, c: int) -> None:
    shapes[pre + "weight"], shapes[pre + "bias"] = (c,), (c,)
    buffers[pre + "running_mean"], buffers[pre + "running_var"], buffers[pre + "num_batches_tracked"] = (c,), (c,), ()


def _res_block(shapes, buffers, pre: str, c: int) -> None:
    """ResidualBlock(use_efficient=True), efficient_layers.py:118-143."""
    shapes[pre + "conv1.depthwise.weight"], shapes[pre + "conv1.pointwise.weight"] = (c, 1, 3, 3), (c, c, 1, 1)
    _bn(shapes, buffers, pre + "conv1.bn.", c)
    shapes[pre + "conv2.0.weight"], shapes[pre + "conv2.1.weight"] = (c, 1, 3, 3), (c, c, 1, 1)
    _bn(shapes, buffers, pre + "conv2.2.", c)


def _cbam(shapes, pre: str, c: int) -> None:
    shapes[pre + "channel_attention.fc.0.weight"] = (c // 16, c)
    shapes[pre + "channel_attention.fc.2.weight"] = (c, c // 16)
    shapes[pre + "spatial_attention.conv.weight"] = (1, 2, 7, 7)


def tconv_mid(cin: int, cout: int, tk: int = 3) -> int:
    """TemporalConv3D's intermediate width, efficient_layers.py:253-257."""
    return max((cin * cout * 9 * tk) // (cin * 9 + cout * tk), cout // 2)


def shapes(in_channels: int = 3, base: int = 64, num_blocks: int = 2) -> "Tuple[Dict[str, tuple], Dict[str, tuple]]":
    """(parameter shapes, buffer shapes) in the reference's state_dict order of names (frame_recovery.py:35-57,124-137,
    183-207,272-309,361-395)."""
    P: Dict[str, tuple] = {}
    Bf: Dict[str, tuple] = {}
    se = "spatial_encoder."
    P[se + "stem.0.weight"] = (base, in_channels + 1, 7, 7)
    _bn(P, Bf, se + "stem.1.", base)
    cin = base
    for si, cout in ((1, base), (2, base * 2), (3, base * 4)):
        idx = 0
        if si > 1:                                            # stride 2 and a channel change: 1x1 conv + BN first
            P[f"{se}stage{si}.0.0.weight"] = (cout, cin, 1, 1)
            _bn(P, Bf, f"{se}stage{si}.0.1.", cout)
            idx = 1
        for b in range(num_blocks):
            _res_block(P, Bf, f"{se}stage{si}.{idx + b}.", cout)
        cin = cout
    _cbam(P, se + "attention.", base * 4)
    te = "temporal_encoder."
    for name, (ci, co) in (("conv1", (in_channels, 64)), ("conv2", (64, 128)), ("conv3", (128, base * 4))):
        mid = tconv_mid(ci, co)
        P[f"{te}{name}.spatial.0.weight"] = (mid, ci, 1, 3, 3)
        _bn(P, Bf, f"{te}{name}.spatial.1.", mid)
        P[f"{te}{name}.temporal.0.weight"] = (co, mid, 3, 1, 1)
        _bn(P, Bf, f"{te}{name}.temporal.1.", co)
    c4 = base * 4
    P["fusion.align.weight"], P["fusion.align.bias"] = (c4, 2 * c4, 1, 1), (c4,)
    P["fusion.attention.0.weight"], P["fusion.attention.0.bias"] = (c4 // 4, c4, 1, 1), (c4 // 4,)
    P["fusion.attention.2.weight"], P["fusion.attention.2.bias"] = (2, c4 // 4, 1, 1), (2,)
    _res_block(P, Bf, "fusion.refine.0.", c4)
    _res_block(P, Bf, "fusion.refine.1.", c4)
    _cbam(P, "fusion.refine.2.", c4)
    for i, (ci, co) in enumerate(((c4, base * 4), (base * 4, base * 2), (base * 2, base), (base, base // 2)), 1):
        P[f"decoder.up{i}.0.weight"] = (ci, co, 4, 4)       # ConvTranspose2d layout [in, out, k, k]
        _bn(P, Bf, f"decoder.up{i}.1.", co)
    P["decoder.final.0.weight"], P["decoder.final.0.bias"] = (in_channels, base // 2, 3, 3), (in_channels,)
    return P, Bf


# ---------------------------------------------------------------------------- layers
def batch_norm(x: torch.Tensor, P: Params, pre: str, training: bool) -> torch.Tensor:
    """nn.BatchNorm2d / BatchNorm3d: statistics over every dimension but the channel one; train = biased batch variance for
    the normalisation, unbiased one into running_var, momentum 0.1."""
    dims = [d for d in range(x.dim()) if d != 1]
    shape = [1, -1] + [1] * (x.dim() - 2)
    if training:
        n = x.numel() // x.shape[1]
        mean, var = x.mean(dim=dims), x.var(dim=dims, unbiased=False)
        with torch.no_grad():
            P[pre + "running_mean"].mul_(1 - BN_MOMENTUM).add_(BN_MOMENTUM * mean.detach())
            P[pre + "running_var"].mul_(1 - BN_MOMENTUM).add_(BN_MOMENTUM * var.detach() * (n / max(n - 1, 1)))
            P[pre + "num_batches_tracked"] += 1
    else:
        mean, var = P[pre + "running_mean"], P[pre + "running_var"]
    inv = torch.rsqrt(var + BN_EPS) * P[pre + "weight"]
    return (x - mean.view(shape)) * inv.view(shape) + P[pre + "bias"].view(shape)


def residual_block(P: Params, pre: str, x: torch.Tensor, training: bool, prec=None) -> torch.Tensor:
    """ResidualBlock.forward, efficient_layers.py:145-151 (conv1 = DepthwiseSeparableConv :62-67).  The depthwise convs are
    fp32 kernels (nvq_dwconv_forward / _wgrad) whatever the precision; their output is stored in x's type."""
    c = x.shape[1]
    x = store(x, prec)                                    # x's gradient: r(r(DwConv dx) + BatchNorm dres), autograd's bf16 add
    y = store(F.conv2d(grad_share(x, prec), P[pre + "conv1.depthwise.weight"], None, padding=1, groups=c), prec)  # _ops.DwConv
    y = store(conv(F.conv2d, y, P[pre + "conv1.pointwise.weight"], prec=prec), prec)                  # _ops.Conv
    y = store(F.relu(batch_norm(y, P, pre + "conv1.bn.", training)), prec)                             # _ops.BatchNorm
    y = store(F.conv2d(y, P[pre + "conv2.0.weight"], None, padding=1, groups=c), prec)                # _ops.DwConv
    y = store(conv(F.conv2d, y, P[pre + "conv2.1.weight"], prec=prec), prec)                           # _ops.Conv
    y = batch_norm(y, P, pre + "conv2.2.", training)
    return store(F.relu(y + x), prec)                     # _ops.BatchNorm(res=x, relu): one rounding of relu(bn + x)


def cbam(P: Params, pre: str, x: torch.Tensor) -> torch.Tensor:
    """CBAM, efficient_layers.py:176-180,200-205,225-228 (fp32 kernels in every precision: _ops.CBAMFn)."""
    hid = F.relu(x.mean(dim=(2, 3)) @ P[pre + "channel_attention.fc.0.weight"].t())
    ca = torch.sigmoid(hid @ P[pre + "channel_attention.fc.2.weight"].t())
    xc = x * ca[:, :, None, None]
    sm = torch.cat([xc.mean(dim=1, keepdim=True), xc.max(dim=1, keepdim=True)[0]], dim=1)
    return xc * torch.sigmoid(F.conv2d(sm, P[pre + "spatial_attention.conv.weight"], None, padding=3))


def spatial_encoder(P: Params, x: torch.Tensor, training: bool, num_blocks: int = 2,
                    prec=None) -> "Tuple[torch.Tensor, List[torch.Tensor]]":
    """SpatialEncoder.forward, frame_recovery.py:83-108: 7x7 stride-2 stem + BN + ReLU + max-pool, three stages, CBAM.
    The stem is an fp32 kernel (nvq_stem7_forward / _wgrad / nvq_stem7_dgrad) whose output is stored as bf16."""
    pre = "spatial_encoder."
    y = store(F.conv2d(x, P[pre + "stem.0.weight"], None, stride=2, padding=3), prec)                 # _ops.Stem7
    y = F.max_pool2d(store(F.relu(batch_norm(y, P, pre + "stem.1.", training)), prec), 3, 2, 1)
    skips = [y]
    for si in (1, 2, 3):
        idx = 0
        if si > 1:                                        # _ops.Subsample2 + _ops.Conv, _ops.BatchNorm
            y = store(conv(F.conv2d, y, P[f"{pre}stage{si}.0.0.weight"], prec=prec, stride=2), prec)
            y = store(batch_norm(y, P, f"{pre}stage{si}.0.1.", training), prec)
            idx = 1
        for b in range(num_blocks):
            y = residual_block(P, f"{pre}stage{si}.{idx + b}.", y, training, prec)
        if si < 3:
            skips.append(y)
    # (_ops.Cast to fp32 in front of the attention: its backward rounds the gradient, the store of y above)
    return cbam(P, pre + "attention.", y), skips


def temporal_conv3d(P: Params, pre: str, x: torch.Tensor, training: bool, prec=None, first: bool = False,
                    time_major: bool = False) -> torch.Tensor:
    """TemporalConv3D.forward, efficient_layers.py:284-294: (1,3,3) conv + BN3d + ReLU, (3,1,1) conv + BN3d + ReLU.
    first: the network's first temporal conv, whose input gradient is the fp32 kernel nvq_head_dgrad(_tc).  time_major: the
    (3,1,1) conv as the time-major layout runs it (three passes accumulating into bf16 storage: _Bf16TemporalAccum)."""
    y = store(conv(F.conv3d, x, P[pre + "spatial.0.weight"], prec=prec, exact_dgrad=first, padding=(0, 1, 1)), prec)
    y = store(F.relu(batch_norm(y, P, pre + "spatial.1.", training)), prec)
    if prec == "bf16_storage" and time_major:
        y = _Bf16TemporalAccum.apply(y, P[pre + "temporal.0.weight"])                                  # _ops.TemporalConv
    else:
        y = store(conv(F.conv3d, y, P[pre + "temporal.0.weight"], prec=prec, padding=(1, 0, 0)), prec)  # _ops.TemporalConvTC
    return store(F.relu(batch_norm(y, P, pre + "temporal.1.", training)), prec)


def temporal_encoder(P: Params, frames: torch.Tensor, training: bool, prec=None, time_major: bool = False) -> torch.Tensor:
    """TemporalEncoder.forward, frame_recovery.py:142-167: (B,T,C,H,W) -> (B,C',H/4,W/4), mean over T at the end (an fp32
    mean of the stored values: _ops.GroupMean / GroupMeanTC)."""
    pre = "temporal_encoder."
    x = frames.permute(0, 2, 1, 3, 4)
    x = F.max_pool3d(temporal_conv3d(P, pre + "conv1.", x, training, prec, True, time_major), (1, 2, 2))
    x = F.max_pool3d(temporal_conv3d(P, pre + "conv2.", x, training, prec, False, time_major), (1, 2, 2))
    return temporal_conv3d(P, pre + "conv3.", x, training, prec, False, time_major).mean(dim=2)


def fusion(P: Params, spatial: torch.Tensor, temporal: torch.Tensor, training: bool, prec=None) -> torch.Tensor:
    """FusionModule.forward, frame_recovery.py:211-257.  The two 'projections' are channel means broadcast to C_out.
    fp32 storage in every precision (1/16 resolution); the 1x1 convs take bf16 operands under MATH_BF16."""
    if spatial.shape[2:] != temporal.shape[2:]:
        temporal = F.interpolate(temporal, size=spatial.shape[2:], mode="bilinear", align_corners=False)
    aligned = conv(F.conv2d, torch.cat([spatial, temporal], dim=1), P["fusion.align.weight"], P["fusion.align.bias"], prec)
    a = F.relu(conv(F.conv2d, aligned, P["fusion.attention.0.weight"], P["fusion.attention.0.bias"], prec))
    attn = torch.softmax(conv(F.conv2d, a, P["fusion.attention.2.weight"], P["fusion.attention.2.bias"], prec), dim=1)
    c = aligned.shape[1]
    sp = spatial.mean(dim=1, keepdim=True).expand(-1, c, -1, -1)        # conv2d with ones / C_in, :244-251
    tp = temporal.mean(dim=1, keepdim=True).expand(-1, c, -1, -1)
    y = aligned + attn[:, 0:1] * sp + attn[:, 1:2] * tp
    ops = "bf16_operands" if prec is not None else None                # no bf16 storage at this resolution
    y = residual_block(P, "fusion.refine.0.", y, training, ops)
    y = residual_block(P, "fusion.refine.1.", y, training, ops)
    return cbam(P, "fusion.refine.2.", y)


def decoder(P: Params, x: torch.Tensor, training: bool, prec=None) -> torch.Tensor:
    """Decoder.forward, frame_recovery.py:311-332 (the skip connections are accepted and ignored there too).  The final conv
    writes fp32 (its input gradient is stored as bf16: the last store)."""
    x = store(x, prec)                                                   # _ops.Cast to the activation type
    for i in (1, 2, 3, 4):
        x = store(conv(F.conv_transpose2d, x, P[f"decoder.up{i}.0.weight"], prec=prec, stride=2, padding=1), prec)  # _ops.ConvT
        x = store(F.relu(batch_norm(x, P, f"decoder.up{i}.1.", training)), prec)
    return torch.tanh(conv(F.conv2d, x, P["decoder.final.0.weight"], P["decoder.final.0.bias"], prec, padding=1))


def frame_recovery_forward(P: Params, corrupted: torch.Tensor, references: torch.Tensor, mask: torch.Tensor = None,
                           training: bool = True, num_blocks: int = 2, prec=None, time_major: bool = False) -> torch.Tensor:
    """FrameRecoveryNet.forward, frame_recovery.py:397-442.  prec: see the module docstring; time_major (with "bf16_storage"):
    the rounding of the HIP network's time-major temporal layout (time_in_channels False) instead of the time-in-channels one."""
    if prec not in PRECISIONS:
        raise ValueError(f"prec must be one of {PRECISIONS}, got {prec!r}")
    B, C, H, W = corrupted.shape
    if mask is None:
        mask = torch.zeros(B, 1, H, W, device=corrupted.device)
    sp, _ = spatial_encoder(P, torch.cat([corrupted, mask], dim=1), training, num_blocks, prec)
    tp = temporal_encoder(P, references, training, prec, time_major)
    rec = decoder(P, fusion(P, sp, tp, training, prec), training, prec)
    if rec.shape[2:] != (H, W):
        rec = F.interpolate(rec, size=(H, W), mode="bilinear", align_corners=False)
    return corrupted * (1 - mask) + rec * mask
