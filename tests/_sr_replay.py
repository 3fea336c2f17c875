"""Replay of every launch of SuperResolutionNet's training step in float64, each on its own stored operands.

The engine keeps every stored activation of a step in `Saved` and, under `_engine.DEBUG_CAPTURE`, the upstream gradient of every
backward launch.  `read_state` turns those into one flat dictionary S of NCHW float64 tensors; `walk_forward` / `walk_backward`
go through the schedule launch by launch, compute with plain torch what the launch stores FROM THE STORED INPUTS OF THAT
LAUNCH (never from a replayed value), and hand (launch, key, value) to an `emit` callback:

  * `Checker` compares the value with S[key] (the GPU tests, and the seeded defects of the CPU test);
  * `Builder` stores the value as S[key], which chains the replay functions into a whole training step (the CPU self-check
    against oracle/sr_oracle.py).

Nothing chains in a check: the masks are the stored ones and every operand is what the kernel read, so the differences left
are the accumulation precision and the roundings of that one launch.

Operand rounding.  In the bf16 math mode the matrix-core kernels (convolutions, their weight gradients, the correlation and
its gradients) round every operand that is not already stored as bf16 to bf16, round-to-nearest-even: the weights always, an
fp32-stored activation or gradient (du, dlogits, dflow, logits ...) too.  `q` is that rounding (`bf16_round`), the identity
in the exact-fp32 mode and in the float64 chain.  The other kernels (depthwise conv, BatchNorm, warp, softmax sum, CBAM, tail)
compute in fp32 on the stored values.

Keys of S (all NCHW float64 unless noted; per-frame tensors hold the T*B images in slot order [centre, others...]):
  frames [B,T,C,H,W]; img8 (the head weight gradient's operand); feat0; dws.k pws.k mean.k invstd.k act.k (k < 2, absent when
  the next depthwise conv evaluates relu(bn(.)) itself); features; corr corr_pad; flow.1 .. flow.4, flow_pad, flowbits.1 .. 3;
  aligned [B,T*F,H,W]; a1 a1bits a2 logits logits_pad attn weighted gap hid ca sm amax (long) sa; rdb.k.x rdb.k.y.i rdb.k.bits.i;
  rdb.NB.x (the last block's output); fused gr out passmask (bool);
  dout du dg dfused drdb.k dagg dweighted dgap_pix dlogits da2 da1 daligned dflow dflow_x.1 .. 3 dcorr dfeat_all dd.k dx.k;
  grad:<parameter name>.
S["meta"]: geometry, the mode flags and kind[key] in {"bf16", "fp32", "f64"} = how the tensor is stored."""
from __future__ import annotations

import os

import torch
import torch.nn.functional as F

from oracle import sr_oracle

GROWTH, LAYERS, CORR_LD, BN_EPS = 32, 5, 96, 1e-5
FLOW_IDX = (0, 2, 4, 6)
FLOW_CH = [81, 128, 64, 32, 2]

# ---- bounds (max-normalised error; none is taken from a measured HIP value)
TOL_BF16 = 5e-3        # one bf16 rounding of a stored result (tests/test_kernels_gpu.py, "one bf16 rounding of the result"):
                       # half an ulp of 8 significant bits is at most 2^-8 = 3.9e-3 of a value
TOL_F32_FWD = 2e-5     # fp32-stored forward result (TOL of tests/test_ops_gpu.py)
TOL_F32_GRAD = 2e-4    # fp32-stored gradient (_check_param_grads of tests/test_submodules_gpu.py)
TOL_F64 = 1e-10        # the float64 chain against the oracle
NEAR_INT = 1e-4        # warp / dflow: pixels whose float64 source coordinate is this close to an integer are left out ...
NEAR_CAP = 0.005       # ... at most this share of a tensor's pixels


def bound(kind: str, bf16_math: bool, n_inner: int, grad: bool) -> float:
    """kind: storage of the result; n_inner: bf16 roundings inside the launch(es) replayed, not counting the stored result's own"""
    if kind == "f64":
        return TOL_F64
    n = (n_inner if bf16_math else 0) + (1 if kind == "bf16" else 0)
    if n:
        return n * TOL_BF16
    return TOL_F32_GRAD if grad else TOL_F32_FWD


# ----------------------------------------------------------------------------- readers
def ident(t):
    return t


def bf16_round(t):
    return t.float().bfloat16().to(torch.float64)


def f64(t):
    return t.detach().to(torch.float64)


def read_nhwc(t, c=None, off=0):
    """channels [off, off + c) of an NHWC tensor -> NCHW float64"""
    c = t.shape[-1] - off if c is None else c
    return f64(t[..., off:off + c]).permute(0, 3, 1, 2).contiguous()


def read_sl(sl):
    """an `Sl` (interleaved channel slice, or the channel prefix of a slice-planar CatBuf) -> NCHW float64"""
    if not sl.plane:
        return read_nhwc(sl.t, sl.c, sl.coff)
    N, H, W, ld = sl.t.shape
    parts = [read_nhwc(sl.t, min(ld, sl.c))]
    for kc in range(ld // 32, sl.c // 32):
        v = torch.as_strided(sl.t, (N, H, W, 32), (H * W * 32, W * 32, 32, 1), sl.t.storage_offset() + kc * sl.plane)
        parts.append(read_nhwc(v))
    return torch.cat(parts, 1)


def read_bits(bits, channels):
    """one-bit masks, int32 [N,H,W] or [N,H,W,words] (bit c % 32 of word c / 32 = channel c) -> bool [N,channels,H,W]"""
    b = bits if bits.dim() == 4 else bits[..., None]
    sh = torch.arange(32, device=b.device, dtype=torch.int32)
    m = ((b[..., None] >> sh) & 1).bool().reshape(*b.shape[:3], -1)[..., :channels]
    return m.permute(0, 3, 1, 2).contiguous()


def pack_bits(mask):
    """inverse of read_bits: bool [N,C,H,W] -> int32 [N,H,W] (C <= 32) or [N,H,W,C / 32]"""
    N, C, H, W = mask.shape
    words = (C + 31) // 32
    m = torch.zeros(N, H, W, words * 32, dtype=torch.int64)
    m[..., :C] = mask.permute(0, 2, 3, 1).long()
    v = (m.view(N, H, W, words, 32) << torch.arange(32)).sum(-1)
    v = torch.where(v >= 2 ** 31, v - 2 ** 32, v).to(torch.int32)
    return v[..., 0].contiguous() if words == 1 else v


def read_amax(a):
    return a.detach().long()


# ----------------------------------------------------------------------------- replay functions (plain torch, float64)
def conv(x, w, b, q, relu=False):
    y = F.conv2d(q(x), q(w), b, padding=w.shape[-1] // 2)
    return F.relu(y) if relu else y


def conv_wgrad(x, dy, wshape, q):
    """weight and bias gradient of conv(x, w) + b for the upstream gradient dy; only the first wshape[1] channels of x count.
    The bias gradient sums dy as it is stored: the matrix-core kernel rounds an fp32-stored dy for the MFMAs only and sums its
    "unrounded values" for the bias (csrc/conv_bf16.hip, the dy staging of conv_wgrad_bf16_kernel)."""
    w = torch.zeros(wshape, dtype=torch.float64, device=x.device, requires_grad=True)
    xq, dyq = q(x[:, :wshape[1]]), q(dy)
    y = F.conv2d(xq, w, None, padding=wshape[-1] // 2)
    dw, = torch.autograd.grad(y, w, dyq)
    return dw, dy.sum(dim=(0, 2, 3))


def conv_dgrad(dy, w, q):
    return F.conv_transpose2d(q(dy), q(w), None, padding=w.shape[-1] // 2)


def head_forward(frames, slots, w, b, q):
    x = torch.cat([frames[:, t] for t in slots], 0)
    return F.relu(F.conv2d(x, q(w), b, padding=1))


def groups(x, T):
    """[T*B, ...] in slot order -> list of the T per-frame groups"""
    return list(x.chunk(T, 0))


def bn_apply(p, mean, invstd, gamma, beta, T):
    """relu(gamma * (p - mean) * invstd + beta) with the per-(frame, channel) statistics [T, C]"""
    out = [F.relu((pg - mean[j][None, :, None, None]) * (invstd[j] * gamma)[None, :, None, None] + beta[None, :, None, None])
           for j, pg in enumerate(groups(p, T))]
    return torch.cat(out, 0)


def bn_stats(p, T):
    mean = torch.stack([pg.mean(dim=(0, 2, 3)) for pg in groups(p, T)])
    var = torch.stack([pg.var(dim=(0, 2, 3), unbiased=False) for pg in groups(p, T)])
    return mean, torch.rsqrt(var + BN_EPS)


def dwconv(x, w):
    return F.conv2d(x, w, None, padding=1, groups=x.shape[1])


def bn_relu_backward(p, gamma, beta, dy, T):
    """backward of relu(batch_norm(p)) with per-frame batch statistics -> (dp, dgamma, dbeta)"""
    pl = p.clone().requires_grad_(True)
    g, b = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    y = torch.cat([F.relu(F.batch_norm(pg, None, None, g, b, True, 0.0, BN_EPS)) for pg in groups(pl, T)], 0)
    return torch.autograd.grad(y, (pl, g, b), dy)


def correlation(x1, x2, q):
    """x1 [NO,..] the reference frames' features, x2 [B,..] the centre frame's (image n of x1 meets n % B of x2)"""
    return sr_oracle.correlation(q(x1), q(x2).repeat(x1.shape[0] // x2.shape[0], 1, 1, 1))


def near_integer(flow):
    """bool [N,H,W]: the source coordinate (x + flow_x, y + flow_y) lies within NEAR_INT of a cell boundary"""
    N, _, H, W = flow.shape
    gx = torch.arange(W, dtype=flow.dtype, device=flow.device)[None, None, :] + flow[:, 0]
    gy = torch.arange(H, dtype=flow.dtype, device=flow.device)[None, :, None] + flow[:, 1]
    return ((gx - gx.round()).abs() < NEAR_INT) | ((gy - gy.round()).abs() < NEAR_INT)


def warp_backward(feat, flow, dout):
    ft, fl = feat.clone().requires_grad_(True), flow.clone().requires_grad_(True)
    return torch.autograd.grad(sr_oracle.warp(ft, fl), (ft, fl), dout)


def tsum(aligned, logits, T):
    B, TF, H, W = aligned.shape
    attn = torch.softmax(logits, dim=1)
    weighted = (aligned.view(B, T, TF // T, H, W) * attn[:, :, None]).sum(dim=1)
    return attn, weighted


def cbam_pool(weighted, ca):
    xc = weighted * ca[:, :, None, None]
    mx = xc.max(dim=1)[0]
    # ties go to the first maximum
    first = (xc == mx[:, None]).float().argmax(dim=1)
    return torch.stack([xc.mean(dim=1), mx], 1), first


def cbam_spatial(P, weighted, ca, sm):
    sa = torch.sigmoid(F.conv2d(sm, P["temporal_aggregator.refine.spatial_attention.conv.weight"], None, padding=3))
    return sa, weighted * ca[:, :, None, None] * sa


def cbam_backward(P, dout, x, ca, sa, sm, amax, gap, hid):
    """backward of out = x * ca * sa from the stored forward tensors -> dx (without the pooled-mean path), dgap_pix, dw7, dw1, dw2"""
    pre = "temporal_aggregator.refine."
    w1, w2 = P[pre + "channel_attention.fc.0.weight"], P[pre + "channel_attention.fc.2.weight"]
    w7 = P[pre + "spatial_attention.conv.weight"].clone().requires_grad_(True)
    C, HW = x.shape[1], x.shape[2] * x.shape[3]
    dpre = (dout * x * ca[:, :, None, None]).sum(1, keepdim=True) * sa * (1 - sa)
    sml = sm.clone().requires_grad_(True)
    dsm, dw7 = torch.autograd.grad(F.conv2d(sml, w7, None, padding=3), (sml, w7), dpre)
    dxc = dout * sa + dsm[:, 0:1] / C
    dxc = dxc + torch.zeros_like(dxc).scatter_(1, amax[:, None], dsm[:, 1:2])
    dx = dxc * ca[:, :, None, None]
    dca = (dxc * x).sum(dim=(2, 3))
    dcpre = dca * ca * (1 - ca)
    dw2 = dcpre.t() @ hid
    dhid = (dcpre @ w2) * (hid > 0)
    dw1 = dhid.t() @ gap
    return dx, (dhid @ w1) / HW, dw7, dw1, dw2


def tsum_backward(dweighted, dgap_pix, aligned, attn, T):
    B, TF, H, W = aligned.shape
    dw = dweighted + dgap_pix[:, :, None, None]
    al = aligned.view(B, T, TF // T, H, W)
    daligned = (dw[:, None] * attn[:, :, None]).reshape(B, TF, H, W)
    s = (dw[:, None] * al).sum(2)
    return daligned, attn * (s - (attn * s).sum(1, keepdim=True))


def tail_forward(P, fused, frames_c, s, q):
    u = conv(fused, P["upsampler.conv.weight"], P["upsampler.conv.bias"], q)
    pre = sr_oracle.bicubic_up(frames_c, s) + F.pixel_shuffle(u, s)
    return pre.clamp(0, 1), pre


# ----------------------------------------------------------------------------- the schedule
def _centre(S):
    m = S["meta"]
    return S["aligned"][:, m["c"] * m["F"]:(m["c"] + 1) * m["F"]]


def walk_forward(S, P, q, emit):
    """every forward launch of _engine.forward, in schedule order"""
    m = S["meta"]
    B, T, H, W, Fc, NB, s, c, slots = m["B"], m["T"], m["H"], m["W"], m["F"], m["NB"], m["s"], m["c"], m["slots"]
    NO = (T - 1) * B
    fe = "feature_extractor."
    emit("head", "feat0", head_forward(S["frames"], slots, P[fe + "head.0.weight"], P[fe + "head.0.bias"], q))
    for k in range(3):
        pre = fe + f"body.{k}."
        L = f"body.{k}"
        if k == 0:
            xin = S["feat0"]
        elif m["bn_on_the_fly"]:
            # the depthwise conv evaluates relu(bn(p)) of the layer before it while it stages p
            xin = bn_apply(S[f"pws.{k - 1}"], S[f"mean.{k - 1}"], S[f"invstd.{k - 1}"], P[fe + f"body.{k - 1}.bn.weight"],
                           P[fe + f"body.{k - 1}.bn.bias"], T)
        else:
            xin = S[f"act.{k - 1}"]
        # evaluated on the fly, relu(bn(p)) is rounded to bf16 once as it is staged ("the same single bf16 rounding as
        # bn_apply_relu_kernel", csrc/dwpw_fwd.hip): one inner rounding in front of the stored result's own
        emit(L, f"dws.{k}", dwconv(xin, P[pre + "depthwise.weight"]), n_inner=1 if (k and m["bn_on_the_fly"]) else 0)
        emit(L, f"pws.{k}", conv(S[f"dws.{k}"], P[pre + "pointwise.weight"], None, q))
        mean, invstd = bn_stats(S[f"pws.{k}"], T)
        emit(L, f"mean.{k}", mean)
        emit(L, f"invstd.{k}", invstd)
        act = bn_apply(S[f"pws.{k}"], S[f"mean.{k}"], S[f"invstd.{k}"], P[pre + "bn.weight"], P[pre + "bn.bias"], T)
        if k == 2:
            emit(L, "features", act + S["feat0"])
        elif not m["bn_on_the_fly"]:
            emit(L, f"act.{k}", act)
    feats = S["features"]
    # (the extractor's last launch writes the centre frame's features straight into their slice of `aligned`: a copy in the
    # chain, one and the same tensor in a HIP state)
    emit("features->aligned", f"aligned[{c}]", feats[:B], into=("aligned", c * Fc, T * Fc))
    if NO:
        emit("correlation", "corr", correlation(feats[B:], feats[:B], q))
        emit("correlation", "corr_pad", torch.zeros_like(S["corr_pad"]), exact=True)
        x = S["corr"]
        for li, idx in enumerate(FLOW_IDX):
            name = f"motion_estimator.flow_net.{idx}."
            y = conv(x, P[name + "weight"], P[name + "bias"], q, relu=idx != 6)
            emit(f"flow.{idx}", f"flow.{li + 1}", y)
            if idx != 6 and f"flowbits.{li + 1}" in S:
                emit(f"flow.{idx}", f"flowbits.{li + 1}", S[f"flow.{li + 1}"] > 0, exact=True)
            x = S[f"flow.{li + 1}"]
        emit("flow.6", "flow_pad", torch.zeros_like(S["flow_pad"]), exact=True)
        for j in range(1, T):
            t = slots[j]
            fl = S["flow.4"][(j - 1) * B:j * B]
            emit(f"warp[{t}]", f"aligned[{t}]", sr_oracle.warp(feats[j * B:(j + 1) * B], fl), into=("aligned", t * Fc, T * Fc),
                 skip=near_integer(fl))
    ta = "temporal_aggregator.attention."
    emit("att.0", "a1", conv(S["aligned"], P[ta + "0.weight"], P[ta + "0.bias"], q, relu=True))
    if "a1bits" in S:
        emit("att.0", "a1bits", S["a1"] > 0, exact=True)
    emit("att.2", "a2", conv(S["a1"], P[ta + "2.weight"], P[ta + "2.bias"], q, relu=True))
    emit("att.4", "logits", conv(S["a2"], P[ta + "4.weight"], P[ta + "4.bias"], q))
    emit("att.4", "logits_pad", torch.zeros_like(S["logits_pad"]), exact=True)
    attn, weighted = tsum(S["aligned"], S["logits"], T)
    emit("tsum", "attn", attn)
    emit("tsum", "weighted", weighted)
    # the pooled mean is formed from the unrounded sum inside the same pass (nvq_tsum_forward's gap_partial)
    emit("tsum+cbam_channel", "gap", weighted.mean(dim=(2, 3)))
    emit("cbam_channel", "hid", F.relu(S["gap"] @ P["temporal_aggregator.refine.channel_attention.fc.0.weight"].t()))
    ca = torch.sigmoid(S["hid"] @ P["temporal_aggregator.refine.channel_attention.fc.2.weight"].t())
    emit("cbam_channel", "ca", ca)
    sm, amax = cbam_pool(S["weighted"], S["ca"])
    emit("cbam_pool", "sm", sm)
    # the argmax of the products as the kernel forms them: in the precision of the stored operands
    lo = torch.float32 if m["kind"].get("ca") == "fp32" else torch.float64
    emit("cbam_pool", "amax", cbam_pool(S["weighted"].to(lo), S["ca"].to(lo))[1], exact=True)
    sa, out = cbam_spatial(P, S["weighted"], S["ca"], S["sm"])
    emit("cbam_spatial", "sa", sa)
    emit("cbam_spatial", "rdb.0.x", out)
    for k in range(NB):
        pre = f"residual_blocks.{k}."
        cat = [S[f"rdb.{k}.x"]]
        for i in range(LAYERS):
            L = f"rdb.{k}.layer.{i}"
            emit(L, f"rdb.{k}.y.{i}", conv(torch.cat(cat, 1), P[pre + f"layers.{i}.0.weight"], P[pre + f"layers.{i}.0.bias"], q,
                                           relu=True))
            if f"rdb.{k}.bits.{i}" in S:
                emit(L, f"rdb.{k}.bits.{i}", S[f"rdb.{k}.y.{i}"] > 0, exact=True)
            cat.append(S[f"rdb.{k}.y.{i}"])
        lff = conv(torch.cat(cat, 1), P[pre + "lff.weight"], P[pre + "lff.bias"], q)
        emit(f"rdb.{k}.lff", f"rdb.{k + 1}.x", 0.2 * lff + S[f"rdb.{k}.x"])
    gr = conv(S[f"rdb.{NB}.x"], P["gff.0.weight"], P["gff.0.bias"], q, relu=True)
    emit("gff", "gr", gr)
    emit("gff", "fused", gr + _centre(S))
    out, pre = tail_forward(P, S["fused"], S["frames"][:, c], s, q)
    emit("tail", "out", out)
    # the clamp mask: 1 where 0 <= pre-clamp <= 1; decided by the stored output wherever that lies strictly inside
    stored = S["out"]
    inside = (stored > 0) & (stored < 1)
    edge = ((pre.abs() < 1e-4) | ((pre - 1).abs() < 1e-4)) & ~inside
    emit("tail", "passmask", inside | ((pre >= 0) & (pre <= 1)), exact=True, skip=edge)


def walk_backward(S, P, q, emit):
    """every backward launch of _engine.backward, in schedule order; every parameter gradient is emitted exactly once"""
    m = S["meta"]
    B, T, H, W, Fc, NB, s, c, slots = m["B"], m["T"], m["H"], m["W"], m["F"], m["NB"], m["s"], m["c"], m["slots"]
    NO = (T - 1) * B
    g = lambda L, name, v, **kw: emit(L, "grad:" + name, v, grad=True, **kw)   # noqa: E731

    # ---- tail
    emit("tail.bwd", "du", F.pixel_unshuffle(S["dout"] * S["passmask"], s), grad=True)
    dw, db = conv_wgrad(S["fused"], S["du"], P["upsampler.conv.weight"].shape, q)
    g("up.wgrad", "upsampler.conv.weight", dw)
    g("up.wgrad", "upsampler.conv.bias", db)
    full = conv_dgrad(S["du"], P["upsampler.conv.weight"], q)
    emit("up.dgrad", "dfused", full, grad=True)
    emit("up.dgrad", "dg", full * (S["gr"] > 0), grad=True)
    # ---- gff
    dw, db = conv_wgrad(S[f"rdb.{NB}.x"], S["dg"], P["gff.0.weight"].shape, q)
    g("gff.wgrad", "gff.0.weight", dw)
    g("gff.wgrad", "gff.0.bias", db)
    top = f"drdb.{NB - 1}" if NB else "dagg"
    emit("gff.dgrad", top, conv_dgrad(S["dg"], P["gff.0.weight"], q), grad=True)
    # ---- dense blocks: LAYERS + 1 stored roundings on the way to the block's input gradient (dy_4 .. dy_0 and the result:
    # _engine._bwd_rdb, the `dy = dcat.y(...)` convs and the `nxt` conv), LAYERS inner ones for a weight gradient
    for k in range(NB - 1, -1, -1):
        pre = f"residual_blocks.{k}."
        ys = [S[f"rdb.{k}.y.{i}"] for i in range(LAYERS)]
        masks = [S[f"rdb.{k}.bits.{i}"] if f"rdb.{k}.bits.{i}" in S else (y > 0) for i, y in enumerate(ys)]
        # a linear map's gradients need the forward VALUES of the concat buffer: the stored ones
        res = rdb_backward(P, k, S[f"rdb.{k}.x"], ys, masks, S[f"drdb.{k}"], q)
        L = f"rdb.{k}.bwd"
        emit(L, f"drdb.{k - 1}" if k else "dagg", res[0], grad=True, n_inner=LAYERS)
        for i in range(LAYERS):
            # dy_i is the (LAYERS - i)-th stored gradient slice of the chain dy_4, dy_3, ...
            g(L, pre + f"layers.{i}.0.weight", res[1 + 2 * i], n_inner=LAYERS - i)
            g(L, pre + f"layers.{i}.0.bias", res[2 + 2 * i], n_inner=LAYERS - i)
        g(L, pre + "lff.weight", res[-2])
        g(L, pre + "lff.bias", res[-1])
    # ---- CBAM
    pre = "temporal_aggregator.refine."
    dx, dgap_pix, dw7, dw1, dw2 = cbam_backward(P, S["dagg"], S["weighted"], S["ca"], S["sa"], S["sm"], S["amax"], S["gap"],
                                                S["hid"])
    emit("cbam.bwd", "dweighted", dx, grad=True)
    emit("cbam.bwd", "dgap_pix", dgap_pix, grad=True)
    g("cbam.bwd", pre + "spatial_attention.conv.weight", dw7)
    g("cbam.bwd", pre + "channel_attention.fc.0.weight", dw1)
    g("cbam.bwd", pre + "channel_attention.fc.2.weight", dw2)
    # ---- softmax-weighted sum, attention convs
    dal, dlogits = tsum_backward(S["dweighted"], S["dgap_pix"], S["aligned"], S["attn"], T)
    emit("tsum.bwd", "dlogits", dlogits, grad=True)
    ta = "temporal_aggregator.attention."
    dw, db = conv_wgrad(S["a2"], S["dlogits"], P[ta + "4.weight"].shape, q)
    g("att.4.wgrad", ta + "4.weight", dw)
    g("att.4.wgrad", ta + "4.bias", db)
    emit("att.4.dgrad", "da2", conv_dgrad(S["dlogits"], P[ta + "4.weight"], q) * (S["a2"] > 0), grad=True)
    dw, db = conv_wgrad(S["a1"], S["da2"], P[ta + "2.weight"].shape, q)
    g("att.2.wgrad", ta + "2.weight", dw)
    g("att.2.wgrad", ta + "2.bias", db)
    a1mask = S["a1bits"] if "a1bits" in S else (S["a1"] > 0)
    emit("att.2.dgrad", "da1", conv_dgrad(S["da2"], P[ta + "2.weight"], q) * a1mask, grad=True)
    dw, db = conv_wgrad(S["aligned"], S["da1"], P[ta + "0.weight"].shape, q)
    g("att.0.wgrad", ta + "0.weight", dw)
    g("att.0.wgrad", ta + "0.bias", db)
    # tsum_backward stores its share of daligned, the att.0 input-gradient conv adds to it (accumulate=True): one inner rounding
    emit("tsum.bwd+att.0.dgrad", "daligned", dal + conv_dgrad(S["da1"], P[ta + "0.weight"], q), grad=True, n_inner=1)
    # ---- motion
    feats = S["features"]
    dfeat = [S["dfused"] + S["daligned"][:, c * Fc:(c + 1) * Fc]]
    if NO:
        dflow = []
        for j in range(1, T):
            t = slots[j]
            fl = S["flow.4"][(j - 1) * B:j * B]
            dft, dfl = warp_backward(feats[j * B:(j + 1) * B], fl, S["daligned"][:, t * Fc:(t + 1) * Fc])
            dfeat.append(dft)
            dflow.append(dfl)
        emit("warp.bwd", "dflow", torch.cat(dflow, 0), grad=True, skip=near_integer(S["flow.4"]))
        dy = S["dflow"]
        for li, idx in reversed(list(enumerate(FLOW_IDX))):
            name = f"motion_estimator.flow_net.{idx}."
            x = S[f"flow.{li}"] if li else S["corr"]
            dw, db = conv_wgrad(x, dy, P[name + "weight"].shape, q)
            g(f"flow.{idx}.wgrad", name + "weight", dw)
            g(f"flow.{idx}.wgrad", name + "bias", db)
            dx = conv_dgrad(dy, P[name + "weight"], q)
            if li:
                mask = S[f"flowbits.{li}"] if f"flowbits.{li}" in S else (x > 0)
                emit(f"flow.{idx}.dgrad", f"dflow_x.{li}", dx * mask, grad=True)
                dy = S[f"dflow_x.{li}"]
            else:
                emit("flow.0.dgrad", "dcorr", dx, grad=True)
                emit("flow.0.dgrad", "dcorr_pad", torch.zeros_like(S["dcorr_pad"]), exact=True)
        # the two correlation gradients finish the feature gradient: the warp's share of the reference frames is stored
        # before it is added (dfeat_oth: one inner rounding), the centre frame's addends are stored tensors themselves
        x1 = q(feats[B:]).clone().requires_grad_(True)
        x2 = q(feats[:B]).clone().requires_grad_(True)
        d1, d2 = torch.autograd.grad(sr_oracle.correlation(x1, x2.repeat(T - 1, 1, 1, 1)), (x1, x2), q(S["dcorr"]))
        # (bilinear weights are continuous across a cell boundary: no pixel of the scattered gradient is left out)
        emit("corr.bwd", "dfeat_all", torch.cat([dfeat[0] + d2, torch.cat(dfeat[1:], 0) + d1], 0), grad=True,
             n_inner=1 if m["kind"].get("dfeat_all") == "bf16" else 0)
    else:
        emit("corr.bwd", "dfeat_all", dfeat[0], grad=True)
    # ---- feature extractor.  Per layer: dp is rounded once on its way to the matrix cores (in LDS in nvq_pw_bn_backward, as a
    # stored tensor in the three-launch form), dd is stored, dx is stored.
    fe = "feature_extractor."
    dcur = S["dfeat_all"]
    for k in (2, 1, 0):
        pre = fe + f"body.{k}."
        L = f"body.{k}.bwd"
        dp, dgam, dbet = bn_relu_backward(S[f"pws.{k}"], P[pre + "bn.weight"], P[pre + "bn.bias"], dcur, T)
        g(L, pre + "bn.weight", dgam)
        g(L, pre + "bn.bias", dbet)
        dw, _ = conv_wgrad(S[f"dws.{k}"], dp, P[pre + "pointwise.weight"].shape, q)
        g(L, pre + "pointwise.weight", dw, n_inner=1)
        emit(L, f"dd.{k}", conv_dgrad(dp, P[pre + "pointwise.weight"], q), grad=True, n_inner=1)
        if k == 0:
            xin = S["feat0"]
        elif m["bn_on_the_fly"]:
            xin = bn_apply(S[f"pws.{k - 1}"], S[f"mean.{k - 1}"], S[f"invstd.{k - 1}"], P[fe + f"body.{k - 1}.bn.weight"],
                           P[fe + f"body.{k - 1}.bn.bias"], T)
        else:
            xin = S[f"act.{k - 1}"]
        wl = torch.zeros_like(P[pre + "depthwise.weight"]).requires_grad_(True)
        dww, = torch.autograd.grad(dwconv(xin, wl), wl, S[f"dd.{k}"])
        # (the x operand evaluated on the fly is rounded to bf16 as it is staged: csrc/dw_bwd.hip, commit(), "the same single
        # bf16 rounding as bn_apply_relu_kernel" - one inner rounding of an fp32-stored sum)
        g(L, pre + "depthwise.weight", dww, n_inner=1 if (k and m["bn_on_the_fly"]) else 0)
        dx = F.conv_transpose2d(S[f"dd.{k}"], P[pre + "depthwise.weight"], None, padding=1, groups=Fc)
        if k == 0 and m["head_fused"]:
            # the skip path and the head's ReLU mask in the same launch: the gradient of the head conv
            dx = (dx + S["dfeat_all"]) * (S["feat0"] > 0)
        emit(L, f"dx.{k}", dx, grad=True)
        dcur = S[f"dx.{k}"]
    dhead = dcur if m["head_fused"] else (dcur + S["dfeat_all"]) * (S["feat0"] > 0)
    dw, db = conv_wgrad(S["img8"], dhead, P[fe + "head.0.weight"].shape, q if m["head_fused"] else ident)
    g("head.wgrad", fe + "head.0.weight", dw)
    g("head.wgrad", fe + "head.0.bias", db)


def rdb_backward(P, k, x, ys, masks, gout, q):
    """One dense block as one linear map with the stored masks, on the STORED concat buffer (layer i's weight gradient is formed
    from the stored [x | y_0 .. y_{i-1}]): the gradient at the block's input and its 12 parameter gradients.  The input-gradient
    convs carry 0.2 * lff^T as a weight of its own (the product is formed first, then rounded like every weight: nvq_rdb_backward_weights);
    the lff weight gradient is 0.2 * the plain one (alpha of its launch).  No cast sits inside the graph: the stored buffer
    needs no operand rounding, the weights are rounded outside."""
    pre = f"residual_blocks.{k}."
    xl = x.clone().requires_grad_(True)
    leaves, feats, reads = [], [xl], []
    for i in range(LAYERS):
        w = P[pre + f"layers.{i}.0.weight"].clone().requires_grad_(True)
        b = P[pre + f"layers.{i}.0.bias"].clone().requires_grad_(True)
        leaves += [w, b]
        wq = q(w.detach()) + (w - w.detach())
        y = F.conv2d(torch.cat(feats, 1), wq, b, padding=1) * masks[i]
        # continue from the stored y_i: same gradient path (y - y.detach() is zero with gradient one)
        feats.append(ys[i] + (y - y.detach()))
    lw = P[pre + "lff.weight"].clone().requires_grad_(True)
    lb = P[pre + "lff.bias"].clone().requires_grad_(True)
    leaves += [lw, lb]
    leff = q(0.2 * lw.detach()) + 0.2 * (lw - lw.detach())
    out = F.conv2d(torch.cat(feats, 1), leff, None) + 0.2 * lb[None, :, None, None] + xl
    return torch.autograd.grad(out, [xl] + leaves, gout)


# ----------------------------------------------------------------------------- emit callbacks
def _write(S, key, want, into):
    if into is None:
        S[key] = want.detach()
    else:
        name, off, total = into
        if name not in S:
            S[name] = torch.zeros(want.shape[0], total, *want.shape[2:], dtype=want.dtype, device=want.device)
        S[name][:, off:off + want.shape[1]] = want.detach()


def _stored(S, key, into, width):
    if into is None:
        return S[key]
    name, off, _ = into
    return S[name][:, off:off + width]


def new_state(frames, F, NB, s, bn_on_the_fly=False, head_fused=False):
    """an empty float64 state for Builder: geometry, the frames, and the zero pads the launches write"""
    B, T, C, H, W = frames.shape
    c = T // 2
    slots = [c] + [t for t in range(T) if t != c]
    NO = (T - 1) * B
    z = lambda n, ch: torch.zeros(n, ch, H, W, dtype=torch.float64)   # noqa: E731
    S = {"meta": dict(B=B, T=T, H=H, W=W, F=F, NB=NB, s=s, c=c, slots=slots, kind={}, bn_on_the_fly=bn_on_the_fly,
                      head_fused=head_fused),
         "frames": frames.double(), "img8": torch.cat([frames[:, t] for t in slots], 0).double(),
         "corr_pad": z(NO, CORR_LD - 81), "flow_pad": z(NO, 2), "logits_pad": z(B, (T + 3) // 4 * 4 - T), "dcorr_pad": z(NO, CORR_LD - 81)}
    return S


class Builder:
    """emit callback that chains the replay: every value becomes the stored tensor the next launch reads"""

    def __init__(self, S):
        self.S = S

    def __call__(self, launch, key, want, grad=False, n_inner=0, exact=False, skip=None, into=None):
        _write(self.S, key, want, into)
        self.S["meta"]["kind"].setdefault(into[0] if into else key, "f64")


class Checker:
    """emit callback that compares every value with the stored tensor; rows: (launch, key, rel, rel_l2, bound, ok)"""

    def __init__(self, S, bf16_math):
        self.S, self.bf16_math, self.rows, self.claimed = S, bf16_math, [], []

    def __call__(self, launch, key, want, grad=False, n_inner=0, exact=False, skip=None, into=None):
        got = _stored(self.S, key, into, want.shape[1] if into else 0)
        if key.startswith("grad:"):
            self.claimed.append(key[5:])
        assert got.shape == want.shape, (launch, key, tuple(got.shape), tuple(want.shape))
        keep = None
        if skip is not None:
            share = skip.double().mean().item()
            assert share <= NEAR_CAP, f"{launch} {key}: {share:.2%} of the pixels left out (cap {NEAR_CAP:.1%})"
            keep = ~skip
            keep = keep[:, None].expand_as(want) if keep.dim() == want.dim() - 1 else keep
        if exact:
            bad = got != want
            if keep is not None:
                bad = bad & keep
            nbad = int(bad.sum())
            self.rows.append((launch, key, float(nbad), float(nbad), 0.0, nbad == 0))
            return
        got, want = got.to(torch.float64), want.detach().to(torch.float64)
        d = got - want
        if keep is not None:
            d, want = d * keep, want * keep
        scale = want.abs().max().clamp_min(1e-300)
        rel = (d.abs().max() / scale).item()
        l2 = (d.norm() / want.norm().clamp_min(1e-300)).item()
        kind = self.S["meta"]["kind"][into[0] if into else key]
        b = bound(kind, self.bf16_math, n_inner, grad)
        self.rows.append((launch, key, rel, l2, b, rel <= b))

    def failures(self):
        return [r for r in self.rows if not r[5]]

    def report(self):
        return "\n".join(f"  {'ok  ' if ok else 'FAIL'} {launch:22s} {key:60s} rel {rel:.2e}  l2 {l2:.2e}  bound {b:.1e}"
                         for launch, key, rel, l2, b, ok in self.rows)

    def worst_by_class(self):
        """{(launch class, storage kind): worst rel} with block / layer / frame indices folded"""
        import re
        out = {}
        for launch, key, rel, l2, b, ok in self.rows:
            cls = re.sub(r"\d+", "*", launch)
            kind = "int" if b == 0.0 else f"{b:.0e}"
            out[(cls, kind)] = max(out.get((cls, kind), 0.0), rel)
        return out


# ----------------------------------------------------------------------------- the HIP run's state
def read_state(net, sv, cap, out, dout):
    """S of one eager training step: sv = out.grad_fn.sv (net.retain_backward_state), cap = the DEBUG_CAPTURE dictionary"""
    g = sv.g
    B, T, H, W, Fc, NB = g.B, g.T, g.H, g.W, g.F, g.NB
    NO = g.NO
    kind = {}
    S = {"meta": dict(B=B, T=T, H=H, W=W, F=Fc, NB=NB, s=g.s, c=g.c, slots=list(g.slots), kind=kind,
                      bn_on_the_fly=sv.acts[0] is sv.pws[0], head_fused=sv.img8 is not None)}

    def put(key, t, val=None):
        kind[key] = "bf16" if t.dtype == torch.bfloat16 else "fp32"
        S[key] = read_nhwc(t) if val is None else val

    S["frames"] = f64(sv.frames)
    # the head weight gradient's x operand: the bf16 frames of the matrix-core form, else the frames themselves (slot order)
    S["img8"] = read_nhwc(sv.img8, g.Cimg) if sv.img8 is not None else torch.cat([S["frames"][:, t] for t in g.slots], 0)
    put("feat0", sv.feat0)
    for k in range(3):
        put(f"dws.{k}", sv.dws[k])
        put(f"pws.{k}", sv.pws[k])
        kind[f"mean.{k}"] = kind[f"invstd.{k}"] = "fp32"
        S[f"mean.{k}"], S[f"invstd.{k}"] = f64(sv.bn_mean[k]), f64(sv.bn_invstd[k])
        if k < 2 and sv.acts[k] is not sv.pws[k]:
            put(f"act.{k}", sv.acts[k])
    put("aligned", sv.aligned)
    c = g.c
    kind["features"] = kind["aligned"]
    S["features"] = torch.cat([S["aligned"][:, c * Fc:(c + 1) * Fc]] + ([read_nhwc(sv.feat_oth)] if NO else []), 0)
    if NO:
        put("corr", sv.flow_acts[0], read_nhwc(sv.flow_acts[0], 81))
        S["corr_pad"] = read_nhwc(sv.flow_acts[0], CORR_LD - 81, 81)
        for li in range(1, 5):
            put(f"flow.{li}", sv.flow_acts[li], read_nhwc(sv.flow_acts[li], FLOW_CH[li]))
            if li < 4 and sv.flow_bits[li] is not None:
                S[f"flowbits.{li}"] = read_bits(sv.flow_bits[li], FLOW_CH[li])
        S["flow_pad"] = read_nhwc(sv.flow_acts[4], 2, 2)
    put("a1", sv.a1)
    if sv.a1_bits is not None:
        S["a1bits"] = read_bits(sv.a1_bits, Fc)
    put("a2", sv.a2)
    put("logits", cap["logits"], read_nhwc(cap["logits"], T))
    S["logits_pad"] = read_nhwc(cap["logits"], g.Tp - T, T)
    put("attn", sv.attn, read_nhwc(sv.attn, T))
    put("weighted", sv.weighted)
    for key, t in (("gap", sv.gap), ("hid", sv.hid), ("ca", sv.ca)):
        kind[key] = "fp32"
        S[key] = f64(t)
    put("sm", sv.sm)
    S["amax"] = read_amax(sv.amax)
    put("sa", sv.sa, f64(sv.sa)[:, None])
    for k in range(NB):
        cat = sv.cats[k]
        kind[f"rdb.{k}.x"] = "bf16" if cat.x().bf16 else "fp32"
        # the x slice through the prefix reader (planar: lead tensor + planes; interleaved: a channel range), the y slices on their own
        whole = read_sl(cat.inp(g.CAT))
        S[f"rdb.{k}.x"] = whole[:, :Fc]
        for i in range(LAYERS):
            kind[f"rdb.{k}.y.{i}"] = kind[f"rdb.{k}.x"]
            S[f"rdb.{k}.y.{i}"] = read_sl(cat.y(i))
            assert torch.equal(S[f"rdb.{k}.y.{i}"], whole[:, Fc + GROWTH * i:Fc + GROWTH * (i + 1)]), "CatBuf readers disagree"
            if sv.bits is not None:
                S[f"rdb.{k}.bits.{i}"] = read_bits(sv.bits[k][i], GROWTH)
    xN = sv.xloc(NB)
    kind[f"rdb.{NB}.x"] = "bf16" if xN.bf16 else "fp32"
    S[f"rdb.{NB}.x"] = read_sl(xN)
    put("fused", sv.fused)
    put("gr", sv.gr)
    kind["out"] = "fp32"
    S["out"] = f64(out)
    S["passmask"] = sv.passmask.bool()
    # ---- backward
    S["dout"] = f64(dout)
    put("du", cap["du"], read_nhwc(cap["du"], g.U))

    def putg(key, name, dtype_of, c=None):
        kind[key] = "bf16" if dtype_of == torch.bfloat16 else "fp32"
        S[key] = read_nhwc(cap[name], c)

    act = sv.act_dtype
    # (the engine's condition for finishing the feature gradient as bf16 in the correlation gradients)
    feat16 = (act == torch.bfloat16 and Fc in (32, 64) and sv.img8 is not None and NO > 0 and sv.aligned.dtype == torch.bfloat16
              and os.environ.get("NVQ_BF16_FEATURE_GRAD", "1") != "0")
    putg("dg", "dg", act)
    putg("dfused", "dfused", torch.bfloat16 if feat16 else torch.float32)
    for k in range(NB):
        putg(f"drdb.{k}", f"drdb{k}", act)
    putg("dagg", "dagg", sv.cbam_dtype if NB else torch.float32)
    putg("dweighted", "dweighted", sv.cbam_dtype)
    kind["dgap_pix"] = "fp32"
    S["dgap_pix"] = f64(cap["dgap_pix"])
    putg("dlogits", "dlogits", torch.float32, T)
    putg("da2", "da2", act)
    putg("da1", "da1", act)
    putg("daligned", "daligned", sv.aligned.dtype)
    if NO:
        putg("dflow", "dflow", torch.float32, 2)
        for li in (1, 2, 3):
            putg(f"dflow_x.{li}", f"dflow_x{li}", act, FLOW_CH[li])
        putg("dcorr", "dcorr", cap["dcorr"].dtype, 81)
        # (fp32 storage: the launch writes pad4(81) = 84 channels, the rest of the 96 is never written)
        S["dcorr_pad"] = read_nhwc(cap["dcorr"], (CORR_LD if cap["dcorr"].dtype == torch.bfloat16 else 84) - 81, 81)
    putg("dfeat_all", "dfeat_all", torch.bfloat16 if feat16 else torch.float32)
    for k in range(3):
        putg(f"dd.{k}", f"dd{k}", act)
        putg(f"dx.{k}", f"dx{k}", act if (k > 0 or sv.img8 is not None) else torch.float32)
    for n, p in net.named_parameters():
        kind["grad:" + n] = "fp32"
        S["grad:" + n] = f64(p.grad)
    return S


def params64(net_or_dict, device=None):
    sd = net_or_dict if isinstance(net_or_dict, dict) else net_or_dict.state_dict()
    return {n: (f64(t).to(device) if device is not None else f64(t)) for n, t in sd.items() if t.is_floating_point()}
