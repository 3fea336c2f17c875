"""Kernel schedule of SuperResolutionNet forward and backward on libnvq.

The op order follows the reference forward (super_resolution.py:327-391); every arithmetic
step is a libnvq kernel launch on the current HIP stream, PyTorch only owns the buffers.
Internal activations are fp32 NHWC.  Frames are processed in "slot" order
[centre, other frames...] so the T feature-extractor calls of the reference become one
batched launch per layer (BatchNorm statistics stay per frame, see nvq_bn_stats).

Dense-block concatenation (torch.cat at super_resolution.py:249,252) never happens: each
block owns one [B,H,W,F+160] buffer, layer i reads channels [0, F+32i) and writes
[F+32i, F+32i+32); the backward accumulates into a gradient buffer of the same layout.
"""
from __future__ import annotations

import os
from typing import Dict, Optional

import torch

from . import _nvq as K
from ._nvq import Sl

GROWTH = 32   # ResidualDenseBlock growth_rate (fixed, super_resolution.py:227)
LAYERS = 5    # ResidualDenseBlock num_layers   (fixed, super_resolution.py:228)
CORR_LD = 96  # 81 correlation channels stored in a 96-channel NHWC buffer (pad = 0)
BN_EPS = 1e-5
BN_MOM = 0.1

_ws_cache: Dict[torch.device, torch.Tensor] = {}

# When set to a dict, forward() stores the flows, the dense blocks' output and the fused features, and backward() the
# intermediate gradients in it (tests / debugging only).
DEBUG_CAPTURE: Optional[dict] = None

_TAIL_ROWS = int(os.environ.get("NVQ_TAIL_ROWS", "0"))   # 4: the four-wave rdb_tail kernel (A/B switch, same results)


def _on(name: str, default: str = "1") -> bool:
    """An A/B switch of the environment, on unless "0"; read at every call (tests and tools/ flip them in a process)."""
    return os.environ.get(name, default) != "0"


def _fused_tail_ok(math: int, x: torch.Tensor, Cimg: int, scale: int) -> bool:
    """nvq_upsampler_tail_forward's domain: bf16 MFMA mode, a bf16-stored input, scale 2..4 with Cimg * scale^2 <= 16 / 32 / 64.
    (The exact-fp32 mode keeps the conv + nvq_shuffle_bicubic_clamp pair; NVQ_FUSED_TAIL=0 selects it in bf16 mode too.)"""
    return (math == K.MATH_BF16 and x.dtype == torch.bfloat16 and scale in (2, 3, 4)
            and Cimg * scale * scale <= {2: 16, 3: 32, 4: 64}[scale] and _on("NVQ_FUSED_TAIL"))


def _allreduce_sum_(t: torch.Tensor, group) -> None:
    """the collective between the reduce and finish phases of a synchronised BatchNorm (nn.SyncBatchNorm)"""
    import torch.distributed as dist
    dist.all_reduce(t, op=dist.ReduceOp.SUM, group=group)


def _capture(name: str, t) -> None:
    """t: a tensor, or a callable producing one (evaluated only while a capture is requested)"""
    if DEBUG_CAPTURE is not None:
        if callable(t):
            t = t()
        DEBUG_CAPTURE[name] = t.clone() if torch.is_tensor(t) else t


class _Packs:
    """The packed weights of one pass.  `prefetch` packs a list of (name, transpose, cin_store, keep) in one launch per 48 jobs
    (K.conv_pack_many); `get` returns such a pack, or packs a single weight the list did not name."""

    def __init__(self, P: Dict[str, torch.Tensor], math: int):
        self.P, self.math, self.done = P, math, {}

    def prefetch(self, reqs) -> None:
        reqs = [r for r in dict.fromkeys(reqs) if r not in self.done]
        outs = K.conv_pack_many([(self.P[n], tr, cs, keep) for n, tr, cs, keep in reqs], self.math)
        self.done.update(zip(reqs, outs))

    def get(self, name: str, transpose: bool, cin_store: int, keep: Optional[int] = None) -> torch.Tensor:
        key = (name, transpose, cin_store, keep)
        wp = self.done.get(key)
        if wp is None:
            wp = self.done[key] = K.conv_pack(self.P[name], transpose, cin_store, keep, math=self.math)
        return wp


def workspace(device) -> torch.Tensor:
    ws = _ws_cache.get(device)
    if ws is None:
        ws = torch.empty(K.wgrad_workspace_bytes() // 4 + (4 << 20), dtype=torch.float32, device=device)
        _ws_cache[device] = ws
    return ws


_ws_multi_cache: Dict = {}
SMALL_STEP_PIXELS = int(os.environ.get("NVQ_SMALL_STEP_PIXELS", str(16 * 128 * 128)))   # batch x H x W up to which a step is launch-bound


def workspace_slots(device, n: int) -> "list[torch.Tensor]":
    """n weight-gradient workspaces that can be in use at the same time (deferred reduces of a dense block: small steps only)"""
    ws = _ws_multi_cache.get((device, n))
    if ws is None:
        k = K.wgrad_workspace_bytes() // 4 + 1024
        flat = torch.empty(n * k, dtype=torch.float32, device=device)
        ws = _ws_multi_cache[(device, n)] = [flat[i * k:(i + 1) * k] for i in range(n)]
    return ws


class _ReduceQueue:
    """Deferred weight-gradient reduces of a launch-bound step: every _wgrad takes the next free workspace slot and leaves its
    reduce in the queue; a full queue (and the end of the pass) is one nvq_wgrad_reduce_batch launch."""
    SLOTS = 8

    def __init__(self, device):
        self.slots = workspace_slots(device, self.SLOTS)
        self.jobs: list = []

    def ws(self) -> torch.Tensor:
        if len(self.jobs) == self.SLOTS:
            self.flush()
        return self.slots[len(self.jobs)]

    def flush(self) -> None:
        K.wgrad_reduce_batch(self.jobs)


class Geometry:
    def __init__(self, frames: torch.Tensor, F: int, nblocks: int, scale: int):
        self.B, self.T, self.Cimg, self.H, self.W = frames.shape
        self.F, self.NB, self.s = F, nblocks, scale
        self.c = self.T // 2
        self.slots = [self.c] + [t for t in range(self.T) if t != self.c]
        self.NI = self.T * self.B
        self.NO = (self.T - 1) * self.B
        self.CAT = F + GROWTH * LAYERS
        # Pixel stride of the dense-block buffers: a multiple of 64 channels, so that every pixel of the bf16 buffer
        # starts on a 128-B line (F=64: 224 -> 256).  The 32-channel (64 B) pieces the conv kernels fetch per pixel
        # and chunk then never share a line with the neighbouring pixel: measured 171 -> 146 us on the cin=192 conv.
        self.CATLD = (self.CAT + 63) // 64 * 64
        self.Tp = K.pad4(self.T)
        self.U = self.Cimg * scale * scale
        self.Up = K.pad4(self.U)
        self.R = F // 16


def _new(dev, *shape, dtype=torch.float32, zero=False):
    return (torch.zeros if zero else torch.empty)(shape, dtype=dtype, device=dev)


class Saved:
    """Everything the backward needs; also the carrier of return_intermediate tensors.  A plain attribute carrier: the
    optional fields have class-level defaults, everything else is set by its producer.
      forward:              g, frames, training, math, act_dtype, aligned, feat_oth, flow_acts, flow_bits, flow (None: T = 1),
                            a1, a2, a1_bits, attn, weighted, cbam_dtype, gap, hid, ca, sm, amax, sa, nblk, cats, resout,
                            planar, bits, fused, gr, passmask, xloc
      _extract:             feat0 (None: forward(features=...), not differentiable), img8, dws, pws, acts, bn_mean,
                            bn_invstd, bn_sync, dw_in, pw_from_dwpw
      light_forward:        frames, training, math, act_dtype, scale, feat0, dws, pws, acts, bn_mean, bn_invstd, bn_sync,
                            passmask, U, Up"""
    feat0 = img8 = flow = None
    bits = a1_bits = flow_bits = None   # one-bit ReLU masks (bf16 training)
    bn_sync = ()                        # (always set by _extract / light_forward) per BatchNorm: (group, stats buffer) or None
    pw_from_dwpw = False                # every extractor layer's p is dwpw_forward's bf16(d W^T)


def _bn_stats(P, pre: str, p, B: int, order, mean, invstd, ws, training: bool, sync, fused: bool = False) -> None:
    """The statistics of BatchNorm `pre` over p's len(order) frame groups -> mean, invstd.  sync = (process group, stats buffer):
    reduce -> all-reduce -> finish (nn.SyncBatchNorm); else training: bn_stats; eval: the running statistics.  fused: the pass
    that made p left the sums (sync) or the statistics (training) already.  Training counts the groups in num_batches_tracked."""
    rmean, rvar = P[pre + "running_mean"], P[pre + "running_var"]
    if sync is not None:
        grp, st = sync
        if not fused:
            K.bn_stats_reduce(p, B, st, ws)
        _allreduce_sum_(st, grp)
        K.bn_stats_finish(st, len(order), order, mean, invstd, rmean, rvar, BN_EPS, BN_MOM)
    elif training and not fused:
        K.bn_stats(p, B, order, mean, invstd, rmean, rvar, ws, BN_EPS, BN_MOM)
    if training:
        P[pre + "num_batches_tracked"].add_(len(order))
    else:
        K.bn_eval_stats(rmean, rvar, len(order), mean, invstd, BN_EPS)


def _extract(P: Dict[str, torch.Tensor], frames: torch.Tensor, slots, F: int, training: bool, math: int,
             act_dtype: torch.dtype, outA: Sl, split_images: int, outB: Optional[Sl], sv, sync=None) -> None:
    """FeatureExtractor.forward (super_resolution.py:40-53) for the T = len(slots) frames of every clip, batched in slot
    order; the features of the first `split_images` images go to outA, the rest to outB.  Saves what backward needs in sv."""
    B, _, _, H, W = frames.shape
    T = len(slots)
    NI = T * B
    dev = frames.device
    ws = workspace(dev)
    feat0 = _new(dev, NI, H, W, F, dtype=act_dtype)
    # bf16 mode: the head's weight gradient runs on the matrix cores (conv_wgrad over the frames as bf16 NHWC-8)
    sv.img8 = _new(dev, NI, H, W, 8, dtype=torch.bfloat16) if (training and K.dwconv_bn_fusable(feat0, F)) else None
    K.head_forward(frames, slots, P["feature_extractor.head.0.weight"], P["feature_extractor.head.0.bias"], feat0,
                   img8=sv.img8, math=math)
    sv.feat0 = feat0
    sv.dws, sv.pws, sv.acts, sv.bn_mean, sv.bn_invstd = [], [], [], [], []
    sv.bn_sync = []
    cur, cur_bn = feat0, None         # cur_bn: BatchNorm + ReLU still to be applied to `cur` (fused into the consumer)
    sv.dw_in = []                     # (tensor, bn) the depthwise conv of layer k was fed with
    fuse_bn = K.dwconv_bn_fusable(feat0, F)
    fused_fwd = fuse_bn and F == 64 and math == K.MATH_BF16 and _on("NVQ_FUSED_DWPW")
    sv.pw_from_dwpw = fused_fwd       # every layer's p is dwpw_forward's bf16(d W^T): the backward may form it again from d
    for k in range(3):
        pre = f"feature_extractor.body.{k}."
        d = _new(dev, NI, H, W, F, dtype=act_dtype)
        p = _new(dev, NI, H, W, F, dtype=act_dtype)
        mean, invstd = _new(dev, T, F), _new(dev, T, F)
        order = [slots.index(t) for t in range(T)]
        grp = sync.get(pre + "bn") if (training and sync) else None
        bsync = (grp, K.new_bn_stats(dev, T, F)) if grp is not None else None
        if fused_fwd and bsync is not None:
            # synchronised BatchNorm: the fused pass leaves the per-frame sums, all ranks add them, then the statistics
            K.dwpw_forward_sums(cur, cur_bn, P[pre + "depthwise.weight"], P[pre + "pointwise.weight"], d, p, B, bsync[1], ws)
        elif fused_fwd:
            # depthwise -> pointwise -> BatchNorm sums in one pass over the tensors (nvq_dwpw_forward)
            K.dwpw_forward(cur, cur_bn, P[pre + "depthwise.weight"], P[pre + "pointwise.weight"], d, p, B,
                           order if training else None, mean, invstd, P[pre + "bn.running_mean"],
                           P[pre + "bn.running_var"], ws, BN_EPS, BN_MOM)
        else:
            K.dwconv_forward(cur, P[pre + "depthwise.weight"], d, bn=cur_bn)
            wp = K.conv_pack(P[pre + "pointwise.weight"], False, F, math=math)
            K.conv_forward(Sl(d), wp, None, Sl(p), 1, math=math)
        _bn_stats(P, pre + "bn.", p, B, order, mean, invstd, ws, training, bsync, fused=fused_fwd)
        sv.bn_sync.append(bsync)
        sv.dw_in.append((cur, cur_bn))
        if k < 2 and fuse_bn:
            # relu(bn(p)) is evaluated by the next depthwise conv (and by its weight gradient) while it stages p
            r, cur_bn = p, (mean, invstd, P[pre + "bn.weight"], P[pre + "bn.bias"], B)
        elif k < 2:
            r, cur_bn = _new(dev, NI, H, W, F, dtype=act_dtype), None
            K.bn_apply_relu(p, B, mean, invstd, P[pre + "bn.weight"], P[pre + "bn.bias"], None, Sl(r), NI)
        else:
            # features = relu(bn(.)) + head features
            r = None
            K.bn_apply_relu(p, B, mean, invstd, P[pre + "bn.weight"], P[pre + "bn.bias"], feat0, outA, split_images, outB)
        sv.dws.append(d); sv.pws.append(p); sv.acts.append(r); sv.bn_mean.append(mean); sv.bn_invstd.append(invstd)
        cur = r


def forward(P: Dict[str, torch.Tensor], frames: torch.Tensor, F: int, nblocks: int, scale: int,
            training: bool, math: int = K.MATH_F32, act_dtype: torch.dtype = torch.float32,
            features: Optional[torch.Tensor] = None, sync: Optional[dict] = None) -> "tuple[torch.Tensor, Saved]":
    """act_dtype: storage type of the conv-internal tensors (dense-block concat buffers, flow-net and attention
    hidden activations and, in backward, their gradients).  torch.bfloat16 needs math == MATH_BF16; every
    tensor a non-conv kernel touches stays fp32.  sync: {BatchNorm holder name: process group} of the synchronised
    BatchNorm layers of a training pass (BucketedNet._sync_bn_groups); their statistics are all-reduced over the group."""
    assert act_dtype == torch.float32 or math == K.MATH_BF16
    g = Geometry(frames, F, nblocks, scale)
    dev = frames.device
    B, T, H, W, NI, NO, c = g.B, g.T, g.H, g.W, g.NI, g.NO, g.c
    ws = workspace(dev)
    sv = Saved()
    sv.g, sv.frames, sv.training, sv.math, sv.act_dtype = g, frames, training, math, act_dtype
    # every forward weight pack of the step in two launches (57 single-pack launches otherwise)
    packs = _Packs(P, math)
    reqs = []
    if NO:
        reqs += [(f"motion_estimator.flow_net.{idx}.weight", False, cs, None)
                 for idx, cs in zip((0, 2, 4, 6), (CORR_LD, K.pad4(128), K.pad4(64), K.pad4(32)))]
    reqs += [("temporal_aggregator.attention.0.weight", False, T * F, None), ("temporal_aggregator.attention.2.weight", False, F, None),
             ("temporal_aggregator.attention.4.weight", False, F, None)]
    for k in range(nblocks):
        reqs += [(f"residual_blocks.{k}.layers.{i}.0.weight", False, F + GROWTH * i, None) for i in range(LAYERS)]
        reqs.append((f"residual_blocks.{k}.lff.weight", False, g.CAT, None))
    reqs += [("gff.0.weight", False, F, None), ("upsampler.conv.weight", False, F, None)]
    packs.prefetch(reqs)

    # ---- feature extractor, all T frames in one batch (slot order)
    # bf16 activation mode: the frames' features (`aligned`: centre frame + warped neighbours, `feat_oth`: the neighbours
    # before warping) are stored as bf16 like every other conv-internal tensor; their non-conv readers (correlation on
    # the matrix cores, warp, softmax-weighted sum) take a storage flag.  NVQ_BF16_FEATURES=0 keeps them fp32.
    feat_dtype = act_dtype if (act_dtype == torch.bfloat16 and math == K.MATH_BF16 and F in (32, 64)
                               and _on("NVQ_BF16_FEATURES")) else torch.float32
    aligned = _new(dev, B, H, W, T * F, dtype=feat_dtype)
    feat_oth = _new(dev, max(NO, 1), H, W, F, dtype=feat_dtype)
    sv.aligned, sv.feat_oth = aligned, feat_oth
    if features is None:
        _extract(P, frames, g.slots, F, training, math, act_dtype, Sl(aligned, F, c * F), B, Sl(feat_oth) if NO else None, sv,
                 sync)
    else:
        # inference with cached per-frame features (extract_features), [T,B,H,W,F] in time order: no extractor launches
        assert not training and tuple(features.shape) == (T, B, H, W, F) and features.dtype == torch.float32
        sv.feat0 = None                                      # marks the state as not differentiable
        aligned[..., c * F:(c + 1) * F].copy_(features[c])
        for j in range(1, T):
            feat_oth[(j - 1) * B:j * B].copy_(features[g.slots[j]])
    center = Sl(aligned, F, c * F)

    # ---- motion: correlation -> flow net -> warp, the T-1 reference frames batched
    if NO:
        # bf16 mode: correlation on the matrix cores, stored as bf16 with the same 96-channel pixel stride (192 B: the 16 pixels a
        # workgroup writes per row are 24 whole 128-B lines, and the flow net's three 32-channel chunks are 64-B pieces that never
        # straddle a line; a 128-channel stride moved a third more bytes through six passes for the same step time)
        corr_bf16 = act_dtype == torch.bfloat16 and F in (32, 64)
        corr = _new(dev, NO, H, W, CORR_LD, dtype=act_dtype if corr_bf16 else torch.float32)
        K.correlation_forward(Sl(feat_oth), center, corr, math=math)
        chans = [81, 128, 64, 32, 2]
        x = Sl(corr, CORR_LD, 0)
        sv.flow_acts = [corr]
        # bf16 mode, training: the hidden layers also leave their ReLU masks as one bit per channel (the input-gradient conv of the
        # layer behind reads 4 bytes per 32 channels instead of the 64-byte activations, as in the dense blocks)
        act_bits = training and act_dtype == torch.bfloat16 and math == K.MATH_BF16 and _on("NVQ_RELU_BITS")
        sv.flow_bits = [None] * 5
        for li, idx in enumerate((0, 2, 4, 6)):
            w = P[f"motion_estimator.flow_net.{idx}.weight"]
            wp = packs.get(f"motion_estimator.flow_net.{idx}.weight", False, x.c)
            last = idx == 6
            y = _new(dev, NO, H, W, K.pad4(chans[li + 1]), dtype=torch.float32 if last else act_dtype)
            # (more than 32 output channels: only the channel-split kernel of a bf16 input writes bits)
            bits = (_new(dev, NO, H, W, chans[li + 1] // 32, dtype=torch.int32)
                    if (act_bits and not last and (x.bf16 or chans[li + 1] <= 32)) else None)
            K.conv_forward(x, wp, P[f"motion_estimator.flow_net.{idx}.bias"], Sl(y, chans[li + 1]), 3,
                           relu=not last, cout_store=K.pad4(chans[li + 1]), math=math, bits=bits, bits_mode=1 if bits is not None else 0)
            sv.flow_acts.append(y)
            sv.flow_bits[li + 1] = bits
            x = Sl(y)
        flow = sv.flow_acts[-1]
        for j in range(1, T):
            t = g.slots[j]
            K.warp_forward(Sl(feat_oth).images((j - 1) * B, j * B), flow[(j - 1) * B:j * B], Sl(aligned, F, t * F))
    sv.flow = sv.flow_acts[-1] if NO else None
    _capture("flow", sv.flow)

    # ---- temporal aggregation
    a1, a2 = _new(dev, B, H, W, F, dtype=act_dtype), _new(dev, B, H, W, F, dtype=act_dtype)
    logits = _new(dev, B, H, W, g.Tp)
    sv.a1_bits = (_new(dev, B, H, W, F // 32, dtype=torch.int32)
                  if (training and act_dtype == torch.bfloat16 and math == K.MATH_BF16 and F % 32 == 0
                      and (aligned.dtype == torch.bfloat16 or F <= 32) and _on("NVQ_RELU_BITS")) else None)
    K.conv_forward(Sl(aligned), packs.get("temporal_aggregator.attention.0.weight", False, T * F),
                   P["temporal_aggregator.attention.0.bias"], Sl(a1), 3, relu=True, math=math, bits=sv.a1_bits,
                   bits_mode=1 if sv.a1_bits is not None else 0)
    K.conv_forward(Sl(a1), packs.get("temporal_aggregator.attention.2.weight", False, F),
                   P["temporal_aggregator.attention.2.bias"], Sl(a2), 3, relu=True, math=math)
    K.conv_forward(Sl(a2), packs.get("temporal_aggregator.attention.4.weight", False, F),
                   P["temporal_aggregator.attention.4.bias"], Sl(logits, T), 3, cout_store=g.Tp, math=math)
    _capture("logits", lambda: logits)
    nblk = K.tsum_blocks(H, W)
    # bf16 activation mode: the aggregated features (the CBAM's input; one write, four reads per step) and the two gradients around
    # the CBAM backward are stored as bf16 like the tensors on either side of them; the pooled sums (GAP, channel mean / max,
    # dca) are formed from the unrounded values inside the kernels.  NVQ_BF16_CBAM=0 keeps them fp32.
    cbam16 = act_dtype == torch.bfloat16 and math == K.MATH_BF16 and nblocks > 0 and _on("NVQ_BF16_CBAM")
    sv.cbam_dtype = torch.bfloat16 if cbam16 else torch.float32
    attn, weighted = _new(dev, B, H, W, g.Tp), _new(dev, B, H, W, F, dtype=sv.cbam_dtype)
    gap_partial = _new(dev, B, nblk, F)
    K.tsum_forward(aligned, logits, T, F, attn, weighted, gap_partial)
    gap, hid, ca = _new(dev, B, F), _new(dev, B, g.R), _new(dev, B, F)
    w1 = P["temporal_aggregator.refine.channel_attention.fc.0.weight"]
    w2 = P["temporal_aggregator.refine.channel_attention.fc.2.weight"]
    w7 = P["temporal_aggregator.refine.spatial_attention.conv.weight"]
    K.cbam_channel(gap_partial, nblk, F, g.R, B, H * W, w1, w2, gap, hid, ca)
    sm, amax, sa = _new(dev, B, H, W, 2), _new(dev, B, H, W, dtype=torch.int32), _new(dev, B, H, W)
    K.cbam_pool(weighted, ca, sm, amax)
    # bf16 mode: slice-planar dense-block buffers (K.CatBuf: x and every growth slice compact tensors of their own, whole
    # 128-B lines written by every layer); NVQ_PLANAR=0 or fp32 storage: one interleaved [B,H,W,CATLD] tensor per block
    planar = act_dtype == torch.bfloat16 and math == K.MATH_BF16 and F in (32, 64, 128) and _on("NVQ_PLANAR")
    cats = [K.CatBuf(dev, B, H, W, F, LAYERS, g.CATLD, act_dtype, planar) for _ in range(nblocks)]
    sv.planar = planar
    # (with no dense blocks the CBAM kernel, an fp32 writer, fills this tensor)
    resout = _new(dev, B, H, W, F, dtype=act_dtype if nblocks else torch.float32)

    def xloc(k):  # where the input of block k / the output of block k-1 lives
        return cats[k].x() if k < nblocks else Sl(resout)
    K.cbam_spatial_apply(weighted, ca, sm, w7, sa, xloc(0))
    sv.a1, sv.a2, sv.attn, sv.weighted = a1, a2, attn, weighted
    sv.gap, sv.hid, sv.ca, sv.sm, sv.amax, sv.sa, sv.nblk = gap, hid, ca, sm, amax, sa, nblk
    sv.cats, sv.resout = cats, resout

    # ---- residual dense blocks
    K.TIMER_TAG = "rdb"
    # bf16 mode: the dense layers also emit their ReLU masks as one bit per channel (4 B per pixel) for the backward
    use_bits = training and act_dtype == torch.bfloat16
    sv.bits = [[_new(dev, B, H, W, dtype=torch.int32) for _ in range(LAYERS)] for _ in range(nblocks)] if use_bits else None
    fuse_tail = (act_dtype == torch.bfloat16 and F == 64        # last dense layer + lff in one pass over the concat buffer
                 and _on("NVQ_FUSE_TAIL"))
    for k in range(nblocks):
        cat = cats[k]
        for i in range(LAYERS - 1 if fuse_tail else LAYERS):
            cin = F + GROWTH * i
            wp = packs.get(f"residual_blocks.{k}.layers.{i}.0.weight", False, cin)
            K.conv_forward(cat.inp(cin), wp, P[f"residual_blocks.{k}.layers.{i}.0.bias"],
                           cat.y(i), 3, relu=True, math=math,
                           bits=sv.bits[k][i] if use_bits else None, bits_mode=1 if use_bits else 0)
        wl = packs.get(f"residual_blocks.{k}.lff.weight", False, g.CAT)
        if fuse_tail:
            i = LAYERS - 1
            cin = F + GROWTH * i
            w3 = packs.get(f"residual_blocks.{k}.layers.{i}.0.weight", False, cin)
            K.rdb_tail_forward(cat.inp(cin), w3, P[f"residual_blocks.{k}.layers.{i}.0.bias"], cat.y(i), wl,
                               P[f"residual_blocks.{k}.lff.bias"], xloc(k + 1), alpha=0.2, res=cat.x(),
                               bits=sv.bits[k][i] if use_bits else None, tile_rows=_TAIL_ROWS)
        else:
            K.conv_forward(cat.inp(g.CAT), wl, P[f"residual_blocks.{k}.lff.bias"], xloc(k + 1), 1, alpha=0.2,
                           res=cat.x(), math=math)

    K.TIMER_TAG = ""
    # ---- global fusion + upsampler tail
    fused, gr = _new(dev, B, H, W, F, dtype=act_dtype), _new(dev, B, H, W, F, dtype=act_dtype)   # conv-to-conv tensors
    _capture("residual", lambda: xloc(nblocks).t[..., :F].float())
    K.conv_forward(xloc(nblocks), packs.get("gff.0.weight", False, F), P["gff.0.bias"], Sl(fused), 3,
                   relu=True, out2=Sl(gr), res=center, math=math)
    _capture("fused", lambda: fused.float())
    out = _new(dev, B, g.Cimg, H * scale, W * scale)
    passmask = _new(dev, B, g.Cimg, H * scale, W * scale, dtype=torch.uint8)
    wup = packs.get("upsampler.conv.weight", False, F)
    if _fused_tail_ok(math, fused, g.Cimg, scale):
        # conv + pixel-shuffle (an LDS transpose in the conv's epilogue) + bicubic skip + clamp: one launch, no `u` tensor
        K.upsampler_tail_forward(Sl(fused), wup, P["upsampler.conv.bias"], frames, c, scale, out, passmask)
    else:
        u = _new(dev, B, H, W, g.Up)
        K.conv_forward(Sl(fused), wup, P["upsampler.conv.bias"], Sl(u, g.U), 3, cout_store=g.Up, math=math)
        K.shuffle_bicubic_clamp(u, frames, c, scale, out, passmask)
    sv.fused, sv.gr, sv.passmask = fused, gr, passmask
    sv.xloc = xloc
    return out, sv


# ----------------------------------------------------------------------------- backward plan (frozen parameters)
class BackwardPlan:
    """What one backward forms.  wgrad: the parameter names whose gradient is written; dx: the stages whose
    input gradient runs (a stage's input gradient is needed iff a parameter of an earlier stage, or the frames, needs a gradient);
    frames: the frames' gradient is formed."""
    __slots__ = ("wgrad", "dx", "frames", "run", "_key")

    def __init__(self, wgrad, dx, frames: bool, stages):
        self.wgrad, self.dx, self.frames = frozenset(wgrad), frozenset(dx), bool(frames)
        self._key = (tuple(sorted(self.wgrad)), self.frames)
        # a stage's backward runs when its input gradient or one of its weight gradients is needed
        self.run = frozenset(st for st, names in stages if st in self.dx or any(n in self.wgrad for n in names))

    @property
    def empty(self) -> bool:
        return not self.wgrad and not self.frames

    def key(self) -> tuple:
        return self._key


def _plan(stages, names_needing_grad, frames_need_grad: bool) -> BackwardPlan:
    need = set(names_needing_grad)
    wgrad, dx = set(), set()
    upstream = bool(frames_need_grad)          # some tensor before the current stage needs a gradient
    for st, names in stages:
        if upstream:
            dx.add(st)
        mine = [n for n in names if n in need]
        wgrad.update(mine)
        upstream = upstream or bool(mine)
    return BackwardPlan(wgrad, dx, frames_need_grad, stages)


def sr_stages(NB: int, T: int) -> "list[tuple[str, list[str]]]":
    """SuperResolutionNet's stages in forward order with their parameter names.  The order is a topological order of the
    forward's dataflow: the extractor's features feed the motion path (correlation -> flow net -> warp) and, through the warp
    and directly (centre frame), the aligned features; so "upstream of a stage" is "earlier in this list".  With T = 1 there is
    no motion path: flow_net has no effect on the output and no gradient is formed for it."""
    fe = "feature_extractor."
    st = [("head", [fe + "head.0.weight", fe + "head.0.bias"])]
    st += [(f"body.{k}", [fe + f"body.{k}.{n}" for n in ("depthwise.weight", "pointwise.weight", "bn.weight", "bn.bias")])
           for k in range(3)]
    if T > 1:
        st += [(f"flow.{i}", [f"motion_estimator.flow_net.{i}.weight", f"motion_estimator.flow_net.{i}.bias"]) for i in (0, 2, 4, 6)]
    ta = "temporal_aggregator."
    st += [(f"att.{i}", [ta + f"attention.{i}.weight", ta + f"attention.{i}.bias"]) for i in (0, 2, 4)]
    st.append(("cbam", [ta + "refine.channel_attention.fc.0.weight", ta + "refine.channel_attention.fc.2.weight",
                        ta + "refine.spatial_attention.conv.weight"]))
    for k in range(NB):
        pre = f"residual_blocks.{k}."
        st.append((f"rdb.{k}", [pre + f"layers.{i}.0.{n}" for i in range(LAYERS) for n in ("weight", "bias")]
                   + [pre + "lff.weight", pre + "lff.bias"]))
    st += [("gff", ["gff.0.weight", "gff.0.bias"]), ("up", ["upsampler.conv.weight", "upsampler.conv.bias"])]
    return st


def backward_plan(names_needing_grad, frames_need_grad: bool, NB: int, T: int) -> BackwardPlan:
    """The backward plan of SuperResolutionNet for a need mask (pure host function)."""
    return _plan(sr_stages(NB, T), names_needing_grad, frames_need_grad)


def light_stages() -> "list[tuple[str, list[str]]]":
    return ([("head", ["net.0.weight", "net.0.bias"])]
            + [(f"block.{j}", [f"net.{k}.{n}" for n in ("depthwise.weight", "pointwise.weight", "bn.weight", "bn.bias")])
               for j, k in enumerate(LIGHT_BLOCKS)]
            + [("up", ["net.6.weight", "net.6.bias"])])


def light_backward_plan(names_needing_grad, frames_need_grad: bool) -> BackwardPlan:
    """The backward plan of LightweightSuperResolution for a need mask."""
    return _plan(light_stages(), names_needing_grad, frames_need_grad)


class _Grads:
    """The gradient targets of a planned backward: get(name) is G[name] when the plan forms that gradient (counted: each is
    written exactly once) and None for a frozen parameter; sink(name) is a throw-away tensor for an output a kernel writes
    unconditionally (the bias next to a trained weight, a BatchNorm affine next to a trained conv)."""

    def __init__(self, G: Dict[str, torch.Tensor], plan: BackwardPlan, P: Dict[str, torch.Tensor]):
        self.G, self.plan, self.P, self.writes = G, plan, P, {}

    def get(self, name: str) -> Optional[torch.Tensor]:
        if name not in self.plan.wgrad:
            return None
        self.writes[name] = self.writes.get(name, 0) + 1
        return self.G[name]

    def sink(self, name: str) -> torch.Tensor:
        g = self.get(name)
        return g if g is not None else torch.empty_like(self.P[name])

    def pair(self, wname: str, bname: Optional[str]):
        """(weight, bias) targets of a conv, None when the plan forms neither; a frozen weight is a sink, a frozen bias None"""
        dw, db = self.get(wname), self.get(bname) if bname else None
        if dw is None and db is None:
            return None
        return (dw if dw is not None else torch.empty_like(self.P[wname])), db

    def check(self) -> None:
        bad = {n: c for n, c in self.writes.items() if c != 1}
        missing = self.plan.wgrad - set(self.writes)
        assert not bad and not missing, f"backward plan: gradients written {bad}, never written {sorted(missing)}"


def _wgrad(x: Sl, cin_w: int, dy: Sl, G: _Grads, wname: str, bname: Optional[str], ws, ksize,
           alpha=1.0, math=K.MATH_F32):
    """ws: the shared workspace (reduce behind the kernel) or a _ReduceQueue (reduce deferred into its next batch).  Nothing runs
    when neither gradient is planned; a frozen bias is not formed, a frozen weight next to a trained bias goes to a sink."""
    t = G.pair(wname, bname)
    if t is None:
        return
    if isinstance(ws, _ReduceQueue):
        K.conv_wgrad(x, cin_w, dy, t[0], t[1], ws.ws(), ksize, alpha=alpha, math=math, defer=ws.jobs)
    else:
        K.conv_wgrad(x, cin_w, dy, t[0], t[1], ws, ksize, alpha=alpha, math=math)


def extract_features(P: Dict[str, torch.Tensor], frames: torch.Tensor, F: int, math: int = K.MATH_F32,
                     act_dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """Per-frame features of a whole video in eval mode (running BatchNorm statistics): frames (B,Tv,C,H,W) ->
    [Tv,B,H,W,F] fp32, to be handed to forward(features=...) window by window (EnhancementEngine.enhance_video)."""
    B, Tv, _, H, W = frames.shape
    out = _new(frames.device, Tv, B, H, W, F)
    for t0 in range(0, Tv, K.MAX_T):                         # the kernels take at most MAX_T frame groups per launch
        n = min(K.MAX_T, Tv - t0)
        part = frames[:, t0:t0 + n].contiguous()
        _extract(P, part, list(range(n)), F, False, math, act_dtype, Sl(out[t0:t0 + n].view(n * B, H, W, F)), n * B, None,
                 Saved())
    return out


class _Bwd:
    """The state of one backward() pass, shared by its stage functions: plain attributes."""

    def __init__(self, P, sv: Saved, dout: torch.Tensor, G, plan: BackwardPlan, deterministic: bool, dinter: Optional[list]):
        g = sv.g
        self.P, self.sv, self.g, self.dout, self.plan, self.deterministic = P, sv, g, dout, plan, deterministic
        self.G = _Grads(G, plan, P)
        self.dinter = dinter if (dinter is not None and any(d is not None for d in dinter)) else None
        self.dev, self.ws = dout.device, workspace(dout.device)
        # Launch-bound steps (small frames: the 64x64 continual-learning step is ~330 dependent launches of a few microseconds):
        # the conv weight gradients leave their partial sums in workspaces of their own and one launch per eight of them does the
        # reduces (nvq_wgrad_reduce_batch; same sums, same order) - ~50 launches less per step.  Large frames keep the reduce
        # behind each kernel, where its partial slabs (up to 56 MB) are still in the last-level cache.
        self.small = g.B * g.H * g.W <= SMALL_STEP_PIXELS and K.TIMER is None
        self.wq = _ReduceQueue(self.dev) if self.small else self.ws
        self.packs = _Packs(P, sv.math)
        # bf16 activation mode with reference frames: the feature gradient is FINISHED by the two correlation gradients, which
        # write it as bf16 (dfeat16, _bwd_motion).  Its terms then never meet in an fp32 accumulator: the upsampler input-gradient
        # conv's second output, the attention path's slice of daligned and the warp gradient are bf16 addends of those last
        # passes (no fp32 gradient tensor, no axpy kernel, no read-modify-write).
        self.feat16 = (sv.math == K.MATH_BF16 and sv.act_dtype == torch.bfloat16 and g.F in (32, 64) and sv.img8 is not None
                       and g.NO > 0 and sv.aligned.dtype == torch.bfloat16 and _on("NVQ_BF16_FEATURE_GRAD"))
        # (set by the stages: du, dg, dcats, dagg, dweighted, dgap_pix, dlogits, daligned, dfeat_all / _c / _c16 / _up, dcur)


def _bwd_up(x: _Bwd) -> bool:
    """upsampler tail: clamp / pixel-shuffle adjoint, the conv's weight and input gradients"""
    g, sv, F = x.g, x.sv, x.g.F
    x.du = _new(x.dev, g.B, g.H, g.W, g.Up)
    K.shuffle_clamp_backward(x.dout, sv.passmask, g.s, x.du)
    _capture("du", lambda: x.du)
    _wgrad(Sl(sv.fused), F, Sl(x.du, g.U), x.G, "upsampler.conv.weight", "upsampler.conv.bias", x.wq, 3, math=sv.math)
    if "up" not in x.plan.dx:
        return False
    # fp32 form: gradient w.r.t. the features of every frame (slot order); the centre frames' part is first written by the
    # upsampler's input-gradient conv (out2 below), the other frames' by the warp backward (overwrite mode), the rest added
    x.dfeat_all = _new(x.dev, g.B, 1, 1, F) if x.feat16 else _new(x.dev, g.NI, g.H, g.W, F)   # (feat16: only a pointer)
    x.dfeat_c = x.dfeat_all[:g.B]
    x.dfeat_c16 = _new(x.dev, g.B, g.H, g.W, F, dtype=torch.bfloat16) if x.feat16 else None
    x.dfeat_up = Sl(x.dfeat_c16 if x.feat16 else x.dfeat_c)   # the centre frames' term as the conv below leaves it
    x.dg = _new(x.dev, g.B, g.H, g.W, F, dtype=sv.act_dtype)
    K.conv_forward(Sl(x.du), x.packs.get("upsampler.conv.weight", True, g.Up, F), None, Sl(x.dg), 3,
                   out2=x.dfeat_up, mask=Sl(sv.gr), mask_c0=0, mask_c1=F, math=sv.math)
    _capture("dg", lambda: x.dg.float())
    return True


def _bwd_gff(x: _Bwd) -> bool:
    g, sv, F, nb = x.g, x.sv, x.g.F, x.g.NB
    _wgrad(sv.xloc(nb), F, Sl(x.dg), x.G, "gff.0.weight", "gff.0.bias", x.wq, 3, math=sv.math)
    if "gff" not in x.plan.dx:    # (the centre features' share, dfeat_up, only matters when the extractor is trained)
        return False
    # gradient buffers of the dense blocks, layout [gout(F) | dy_4 | dy_3 | dy_2 | dy_1 | dy_0] (ping-pong)
    x.dcats = [K.CatBuf(x.dev, g.B, g.H, g.W, F, LAYERS, g.CATLD, sv.act_dtype, sv.planar) for _ in range(2)] if nb else []
    x.dagg = _new(x.dev, g.B, g.H, g.W, F, dtype=sv.cbam_dtype)
    gout = x.dcats[(nb - 1) & 1].x() if nb else Sl(x.dagg)
    K.conv_forward(Sl(x.dg), x.packs.get("gff.0.weight", True, F, F), None, gout, 3, math=sv.math)
    _capture("dfused", lambda: x.dfeat_up.t.float())
    _capture("dres", lambda: gout.t[..., :F].float())
    return True


def _bwd_rdb(x: _Bwd) -> bool:
    """residual dense blocks, last to first, in mirror form (see nvq_rdb_backward_weights)"""
    g, sv, P, G, plan, math = x.g, x.sv, x.P, x.G, x.plan, x.sv.math
    F, nb = g.F, g.NB
    K.TIMER_TAG = "rdb"
    # the gout channels of the mirror-form convs only carry the 1x1 lff^T term: the bf16 kernels skip their other taps
    ctr = F if (math == K.MATH_BF16 and F % 32 == 0) else 0
    # blocks whose backward runs: a suffix k0 .. nb-1 (an upstream need of block k is one of block k + 1)
    ran = [k for k in range(nb) if f"rdb.{k}" in plan.run]
    assert ran == list(range(nb - len(ran), nb))
    # the combined weights of those blocks, then their 6 packs each in one launch
    reqs = []
    for k in ran:
        pre = f"residual_blocks.{k}."
        wb, wbx = K.rdb_backward_weights(P[pre + "lff.weight"], [P[pre + f"layers.{i}.0.weight"] for i in range(LAYERS)], F)
        reqs += [(wb[j], False, F + GROWTH * j, None) for j in range(LAYERS)] + [(wbx, False, g.CAT, None)]
    mirror = K.conv_pack_many(reqs, math)
    for j, k in reversed(list(enumerate(ran))):
        cat, dcat = sv.cats[k], x.dcats[k & 1]
        pre = f"residual_blocks.{k}."
        gout = dcat.x()
        _capture(f"drdb{k}", lambda: gout.t[..., :F].float())
        _wgrad(cat.inp(g.CAT), g.CAT, gout, G, pre + "lff.weight", pre + "lff.bias", x.wq, 1, alpha=0.2, math=math)
        wpb = mirror[j * (LAYERS + 1):(j + 1) * (LAYERS + 1)]     # packs of Wb_4 .. Wb_0, Wb_x
        # dy_i is needed for the block's own input gradient or for the weight gradient of layer i or a layer below it
        lowest = 0 if f"rdb.{k}" in plan.dx else min(
            [i for i in range(LAYERS) if pre + f"layers.{i}.0.weight" in plan.wgrad or pre + f"layers.{i}.0.bias" in plan.wgrad],
            default=LAYERS)
        for i in range(LAYERS - 1, lowest - 1, -1):
            cinb = F + GROWTH * (LAYERS - 1 - i)            # channels [0, cinb) = gout, dy_4 .. dy_{i+1}
            dy = dcat.y(LAYERS - 1 - i)                      # slot of dy_i (channels [cinb, cinb + 32) of the buffer)
            if sv.bits is not None:
                K.conv_forward(dcat.inp(cinb), wpb[LAYERS - 1 - i], None, dy, 3,
                               math=math, bits=sv.bits[k][i], bits_mode=2, center_cin=ctr)
            else:
                K.conv_forward(dcat.inp(cinb), wpb[LAYERS - 1 - i], None, dy, 3,
                               mask=cat.y(i), mask_c0=0, mask_c1=GROWTH, math=math, center_cin=ctr)
            cin = F + GROWTH * i
            _wgrad(cat.inp(cin), cin, dy, G, pre + f"layers.{i}.0.weight", pre + f"layers.{i}.0.bias", x.wq, 3, math=math)
        if f"rdb.{k}" not in plan.dx:
            break
        nxt = x.dcats[(k - 1) & 1].x() if k > 0 else Sl(x.dagg)
        K.conv_forward(dcat.inp(g.CAT), wpb[LAYERS], None, nxt, 3, res=gout, math=math, center_cin=ctr)
    K.TIMER_TAG = ""
    return "cbam" in plan.run


def _bwd_cbam(x: _Bwd) -> bool:
    g, sv, P, G, dxs = x.g, x.sv, x.P, x.G, x.plan.dx
    F = g.F
    dprev = Sl(x.dagg)
    if x.dinter is not None:
        # `aggregated` (the CBAM's output, block 0's input): its gradient is complete here
        K.inject_nchw([(dprev, [x.dinter[2 * g.T]])])
    _capture("dagg", lambda: dprev.t[..., dprev.coff:dprev.coff + F].float())
    fc0, fc2 = "temporal_aggregator.refine.channel_attention.fc.0.weight", "temporal_aggregator.refine.channel_attention.fc.2.weight"
    w7 = "temporal_aggregator.refine.spatial_attention.conv.weight"
    dpre = _new(x.dev, g.B, g.H, g.W)
    K.cbam_bwd_spatial_pre(dprev, sv.weighted, sv.ca, sv.sa, dpre)
    dsm = _new(x.dev, g.B, g.H, g.W, 2)
    # (frozen CBAM weights: the _ex forms, the same dsm / dgap_pix without the weight gradients)
    K.cbam_bwd_spatial_conv(dpre, sv.sm, P[w7], dsm, G.get(w7), x.ws)
    fc_frozen = fc0 not in x.plan.wgrad and fc2 not in x.plan.wgrad
    if "cbam" not in dxs and fc_frozen:
        return False
    x.dweighted = _new(x.dev, g.B, g.H, g.W, F, dtype=sv.cbam_dtype)
    dca_partial = _new(x.dev, g.B, sv.nblk, F)
    K.cbam_bwd_scale(dprev, sv.weighted, sv.ca, sv.sa, dsm, sv.amax, x.dweighted, dca_partial)
    x.dgap_pix = _new(x.dev, g.B, F)
    dw1, dw2 = (None, None) if fc_frozen else (G.sink(fc0), G.sink(fc2))   # (one frozen: the full form, the other into a sink)
    K.cbam_bwd_channel(dca_partial, sv.nblk, F, g.R, g.B, g.H * g.W, P[fc0], P[fc2], sv.gap, sv.hid, sv.ca, dw1, dw2, x.dgap_pix)
    _capture("dgap_pix", lambda: x.dgap_pix)
    return "cbam" in dxs


def _bwd_attention(x: _Bwd) -> bool:
    """softmax-weighted sum and the three attention convs -> daligned (with the intermediates' gradients injected)"""
    g, sv, G, dxs, packs, math = x.g, x.sv, x.G, x.plan.dx, x.packs, x.sv.math
    F, T, c = g.F, g.T, g.c
    x.daligned = _new(x.dev, g.B, g.H, g.W, T * F, dtype=sv.aligned.dtype)   # stored like `aligned` (bf16 in the bf16 mode)
    x.dlogits = _new(x.dev, g.B, g.H, g.W, g.Tp)
    K.tsum_backward(x.dweighted, x.dgap_pix, sv.aligned, sv.attn, T, F, x.daligned, x.dlogits)
    pre = "temporal_aggregator.attention."
    _wgrad(Sl(sv.a2), F, Sl(x.dlogits, T), G, pre + "4.weight", pre + "4.bias", x.wq, 3, math=math)
    if "att.4" in dxs:
        da2 = _new(x.dev, g.B, g.H, g.W, F, dtype=sv.act_dtype)
        K.conv_forward(Sl(x.dlogits), packs.get(pre + "4.weight", True, g.Tp, F), None, Sl(da2), 3,
                       mask=Sl(sv.a2), mask_c0=0, mask_c1=F, math=math)
        _capture("da2", lambda: da2.float())
        _wgrad(Sl(sv.a1), F, Sl(da2), G, pre + "2.weight", pre + "2.bias", x.wq, 3, math=math)
    if "att.2" in dxs:
        da1 = _new(x.dev, g.B, g.H, g.W, F, dtype=sv.act_dtype)
        if sv.a1_bits is not None:
            K.conv_forward(Sl(da2), packs.get(pre + "2.weight", True, F, F), None, Sl(da1), 3, math=math, bits=sv.a1_bits, bits_mode=2)
        else:
            K.conv_forward(Sl(da2), packs.get(pre + "2.weight", True, F, F), None, Sl(da1), 3,
                           mask=Sl(sv.a1), mask_c0=0, mask_c1=F, math=math)
        _capture("da1", lambda: da1.float())
        _wgrad(Sl(sv.aligned), T * F, Sl(da1), G, pre + "0.weight", pre + "0.bias", x.wq, 3, math=math)
    if "att.0" not in dxs:
        # nothing before the attention convs needs a gradient: no motion or extractor backward
        return False
    K.conv_forward(Sl(da1), packs.get(pre + "0.weight", True, F, T * F), None, Sl(x.daligned), 3, accumulate=True, math=math)
    if x.dinter is not None:
        # `aligned[t]` into slice t; `features[c]` (the same tensor in the reference) into slice c too, which reaches the centre
        # frame's feature gradient in both forms of _bwd_motion (axpy_slice / the correlation gradient's addend)
        K.inject_nchw([(Sl(x.daligned, F, t * F), [x.dinter[T + t]] + ([x.dinter[c]] if t == c else [])) for t in range(T)])
    return True


def _bwd_motion(x: _Bwd) -> bool:
    """the rest of the feature gradient (fp32 dfeat_all or bf16 dfeat16, _Bwd.feat16): warp, flow net, correlation"""
    g, sv, math, feat16 = x.g, x.sv, x.sv.math, x.feat16
    B, T, F, c, NO = g.B, g.T, g.F, g.c, g.NO
    daligned = x.daligned
    if not feat16:
        K.axpy_slice(Sl(x.dfeat_c), Sl(daligned, F, c * F))
    _capture("dweighted", lambda: x.dweighted.float())
    _capture("dlogits", x.dlogits)
    _capture("daligned", daligned)
    if not NO:
        return True
    # (feat16: the reference frames' term from the warp leaves as bf16 too and is an addend of the correlation gradient's pass)
    dfeat_oth = _new(x.dev, NO, g.H, g.W, F, dtype=torch.bfloat16) if feat16 else x.dfeat_all[B:]
    dflow = _new(x.dev, NO, g.H, g.W, 4)
    for j in range(1, T):
        lo, hi = (j - 1) * B, j * B
        K.warp_backward(Sl(daligned, F, g.slots[j] * F), Sl(sv.feat_oth).images(lo, hi), sv.flow[lo:hi],
                        Sl(dfeat_oth).images(lo, hi), dflow[lo:hi], overwrite=True, deterministic=bool(x.deterministic))
    acts = sv.flow_acts          # [corr(96), f1(128), f2(64), f3(32), flow(4)]
    chans = [81, 128, 64, 32, 2]
    dy_t, dy_c = dflow, 2
    for li, idx in reversed(list(enumerate((0, 2, 4, 6)))):
        x_t = acts[li]
        name = f"motion_estimator.flow_net.{idx}."
        x_sl = Sl(x_t) if li > 0 else Sl(x_t, CORR_LD, 0)
        _wgrad(x_sl, chans[li], Sl(dy_t, dy_c), x.G, name + "weight", name + "bias", x.wq, 3, math=math)
        if f"flow.{idx}" not in x.plan.dx:
            break
        wp = x.packs.get(name + "weight", True, dy_t.shape[-1], chans[li])
        dx_t = _new(x.dev, NO, g.H, g.W, x_t.shape[-1], dtype=sv.act_dtype if li > 0 else x_t.dtype)
        if li > 0 and sv.flow_bits[li] is not None:
            K.conv_forward(Sl(dy_t), wp, None, Sl(dx_t, chans[li]), 3, math=math, bits=sv.flow_bits[li], bits_mode=2)
        elif li > 0:
            K.conv_forward(Sl(dy_t), wp, None, Sl(dx_t, chans[li]), 3, mask=Sl(x_t), mask_c0=0,
                           mask_c1=chans[li], math=math)
        else:
            # gradient of the correlation volume: the bf16 volume's 96-channel rows are written whole (zeros behind the
            # 81 real channels) - a row of 84 channels would leave lines half written (fill reads)
            full = dx_t.shape[-1] if dx_t.dtype == torch.bfloat16 else K.pad4(chans[li])
            K.conv_forward(Sl(dy_t), wp, None, Sl(dx_t, chans[li]), 3, cout_store=full, math=math)
        _capture(f"dflow_x{li}", lambda: dx_t.float())
        dy_t, dy_c = dx_t, chans[li]
    dcorr = dy_t
    _capture("f1", acts[1])
    _capture("dflow", dflow)
    if "flow.0" not in x.plan.dx:
        # a trained flow net in front of a frozen extractor (and frames without a gradient): the pass ends here
        return False
    _capture("dcorr", dcorr)
    if x.dinter is not None:
        # `features[t]`, t != c: the warp gradient has written its slot; the correlation gradients add to it / read it next
        K.inject_nchw([(Sl(dfeat_oth).images((j - 1) * B, j * B), [x.dinter[g.slots[j]]]) for j in range(1, T)])
    center = Sl(sv.aligned, F, c * F)
    # The two correlation gradients are the LAST terms of the feature gradient.  bf16 activation mode: they write the finished
    # sum as bf16 (dfeat16) instead of back into the fp32 accumulator - the extractor's backward reads it three times
    # (BatchNorm sums, pointwise backward, the skip add of the first depthwise layer) at half the bytes, like every other
    # gradient it consumes.  The second one is the gradient w.r.t. the centre frame's features: the T - 1 reference frames in
    # one pass.
    if feat16:
        dfeat16 = _new(x.dev, g.NI, g.H, g.W, F, dtype=torch.bfloat16)
        K.correlation_backward(1, dcorr, center, Sl(x.dfeat_c), False, math=math, out16=dfeat16[B:], addends=(Sl(dfeat_oth),))
        K.correlation_backward(2, dcorr, Sl(sv.feat_oth), Sl(x.dfeat_c), False, math=math, groups=T - 1, out16=dfeat16[:B],
                               addends=(Sl(x.dfeat_c16), Sl(daligned, F, c * F)))
        x.dfeat_all = dfeat16
    else:
        K.correlation_backward(1, dcorr, center, Sl(dfeat_oth), True, math=math)
        K.correlation_backward(2, dcorr, Sl(sv.feat_oth), Sl(x.dfeat_c), True, math=math, groups=T - 1)
    return True


def _bn_relu_bwd(P, G: _Grads, pre: str, dy, p, B: int, mean, invstd, training: bool, sync, ws) -> torch.Tensor:
    """BatchNorm + ReLU backward of the plain (unfused) block `pre` -> dp, the gradient at the pointwise conv's output.
    sync = (process group, forward stats buffer): the sums of every rank, dp from them and the forward's global count."""
    gamma, beta = P[pre + "bn.weight"], P[pre + "bn.bias"]
    dp = torch.empty_like(p)
    if sync is None:
        K.bn_relu_backward(dy, p, B, mean, invstd, gamma, beta, training, dp, G.sink(pre + "bn.weight"), G.sink(pre + "bn.bias"), ws)
        return dp
    bsums = _new(p.device, mean.numel() * 2, dtype=torch.float64)
    K.bn_relu_backward_reduce(dy, p, B, mean, invstd, gamma, beta, bsums, G.get(pre + "bn.weight"), G.get(pre + "bn.bias"), ws)
    _allreduce_sum_(bsums, sync[0])
    K.bn_relu_backward_finish(dy, p, B, mean, invstd, gamma, beta, bsums, K.bn_counts(sync[1], *mean.shape), dp)
    return dp


def _bwd_body(x: _Bwd) -> bool:
    """feature extractor body (all frames batched), layers 2, 1, 0 -> dcur, the gradient at the head conv's output"""
    g, sv, P, G, ws, run = x.g, x.sv, x.P, x.G, x.ws, x.plan.run
    B, T, F, math, act = g.B, g.T, g.F, sv.math, sv.act_dtype
    if "body.2" not in run:                     # (T = 1: no motion path, the attention convs' need decides)
        return False
    _capture("dfeat_all", lambda: x.dfeat_all.float())
    dcur = x.dcur = x.dfeat_all
    # (built and measured, off by default: with the sums in it the depthwise backward only fits its registers with two instead
    # of five unrolled rows, and the step is 0.2 ms SLOWER than with the separate 0.54 ms reduce passes it replaces; never with
    # a synchronised layer, whose sums are all-reduced between its reduce and finish phases)
    fuse_sums = _on("NVQ_FUSED_BN_SUMS", "0") and not any(sv.bn_sync)
    sums = None      # (BatchNorm-backward sums, dgamma, dbeta) of layer k, when the depthwise backward of layer k + 1 left them
    for k in (2, 1, 0):
        pre = f"feature_extractor.body.{k}."
        if f"body.{k}" not in run:                # the layers below need nothing either
            break
        need_dx = f"body.{k}" in x.plan.dx
        p, d, mean, invstd, bsync = sv.pws[k], sv.dws[k], sv.bn_mean[k], sv.bn_invstd[k], sv.bn_sync[k]
        gamma, beta, wpw = P[pre + "bn.weight"], P[pre + "bn.bias"], P[pre + "pointwise.weight"]
        fused = math == K.MATH_BF16 and act == p.dtype == d.dtype == torch.bfloat16 and F == 64
        dd = torch.empty_like(p)
        # the pass behind the BatchNorm sums forms p again from the d tile it stages anyway (one tensor pass fewer, the
        # same bits) when the forward made p from this d and this weight in the fused pass
        recompute = fused and sv.pw_from_dwpw and _on("NVQ_PW_RECOMPUTE")
        if not (fused and _on("NVQ_FUSED_PW_BWD")):
            dp = _bn_relu_bwd(P, G, pre, dcur, p, B, mean, invstd, sv.training, bsync, ws)
            _wgrad(Sl(d), F, Sl(dp), G, pre + "pointwise.weight", None, x.wq, 1, math=math)
            # (also when nothing reads dd: frozen depthwise weight, no input gradient needed)
            K.conv_forward(Sl(dp), K.conv_pack(wpw, True, F, F, math=math), None, Sl(dd), 1, math=math)
        elif bsync is not None:
            # synchronised BatchNorm: {sum g, sum g xhat} of every rank, dx from the global sums and the forward's global count
            bsums = _new(dd.device, T * 2 * F, dtype=torch.float64)
            K.pw_bn_backward_reduce(dcur, p, B, mean, invstd, gamma, beta, bsums, G.get(pre + "bn.weight"), G.get(pre + "bn.bias"), ws)
            _allreduce_sum_(bsums, bsync[0])
            K.pw_bn_backward_finish(dcur, p, d, B, mean, invstd, gamma, beta, wpw, dd, G.get(pre + "pointwise.weight"), bsums,
                                    K.bn_counts(bsync[1], T, F), ws, recompute=recompute)
        else:
            # BatchNorm backward + the pointwise conv's input and weight gradients in one pass behind the BatchNorm sums: dp is
            # formed in LDS and never stored (nvq_pw_bn_backward; a frozen pointwise weight or BatchNorm affine: the _ex form)
            bn_sums, dgam, dbet = sums or (None, G.get(pre + "bn.weight"), G.get(pre + "bn.bias"))
            K.pw_bn_backward(dcur, p, d, B, mean, invstd, gamma, beta, sv.training, wpw, dd, dgam, dbet,
                             G.get(pre + "pointwise.weight"), ws, sums_in=bn_sums, recompute=recompute)
        _capture(f"dd{k}", lambda: dd.float())
        xin, xin_bn = sv.dw_in[k]
        dww, sums = G.get(pre + "depthwise.weight"), None
        if fused and k > 0 and xin.dtype == torch.bfloat16 and _on("NVQ_FUSED_DW_BWD"):
            # the depthwise conv's input gradient and weight gradient from one staged tile (nvq_dwconv_backward).  Not for the
            # first layer: with the skip-path add and the head's ReLU mask in its epilogue the one-tile kernel takes as long as
            # the two launches below (2.53 vs 2.54 ms: the epilogue operands are loaded where they are used, by 8 waves per CU).
            # A frozen depthwise weight: dx alone (dweight None -> the _ex form)
            if not need_dx and dww is None:
                break
            dx = torch.empty_like(dd)
            if fuse_sums and sv.training and need_dx and _on("NVQ_FUSED_PW_BWD"):
                # ... and the backward sums of layer k - 1's BatchNorm: this kernel holds its input (xin) and the gradient of
                # its activation (dx), so the next pw_bn_backward needs no reduce pass of its own
                prev = f"feature_extractor.body.{k - 1}."
                sums = (_new(dd.device, T, 2, F), G.sink(prev + "bn.weight"), G.sink(prev + "bn.bias"))
            bn_sums, dgam, dbet = sums or (None, None, None)
            K.dwconv_backward(xin, xin_bn, dd, P[pre + "depthwise.weight"], dx, dww, ws, bn_sums=bn_sums, bn_dgamma=dgam, bn_dbeta=dbet)
        else:
            if dww is not None:
                K.dwconv_wgrad(xin, dd, dww, ws, bn=xin_bn)
            if not need_dx:
                break
            # first layer, bf16 mode: dx + skip path, ReLU-masked by the head features: the gradient of the head conv, as bf16
            add, mask = (x.dfeat_all, sv.feat0) if (k == 0 and sv.img8 is not None) else (None, None)
            dx = torch.empty_like(dd, dtype=act if (k > 0 or add is not None) else torch.float32)
            K.dwconv_forward(dd, P[pre + "depthwise.weight"], dx, flip=True, add=add, mask=mask)
        _capture(f"dx{k}", lambda: dx.float())
        dcur = x.dcur = dx
    return True


def _bwd_head(x: _Bwd) -> bool:
    g, sv, bname = x.g, x.sv, "feature_extractor.head.0.bias"
    hw = x.G.pair("feature_extractor.head.0.weight", bname) if "head" in x.plan.run else None
    if hw is not None and sv.img8 is not None:
        K.conv_wgrad(Sl(sv.img8), g.Cimg, Sl(x.dcur), hw[0], hw[1], x.ws, 3, math=sv.math)
    elif hw is not None:
        # the skip path of  feat = body(h) + h  is summed inside the head kernel (dout2)
        K.head_wgrad(sv.frames, g.slots, x.dcur, sv.feat0, hw[0], hw[1] if hw[1] is not None else x.G.sink(bname), x.ws,
                     dout2=x.dfeat_all)
    return True


# reverse sr_stages order; each returns whether the pass continues upstream (False: nothing further is needed)
_BWD_STAGES = (_bwd_up, _bwd_gff, _bwd_rdb, _bwd_cbam, _bwd_attention, _bwd_motion, _bwd_body, _bwd_head)


def backward(P: Dict[str, torch.Tensor], sv: Saved, dout: torch.Tensor, G: Dict[str, torch.Tensor],
             deterministic: bool = False, dframes: Optional[torch.Tensor] = None, plan: Optional[BackwardPlan] = None,
             dinter: Optional[list] = None) -> None:
    """Write the gradient of every parameter of the plan into G[name] (each exactly once, overwrite).  deterministic: the warp
    gradient without float atomics for any flow (every other kernel of the backward sums in a fixed order already).
    dframes (B,T,Cimg,H,W) fp32: also write the gradient w.r.t. the input frames (overwrite) - two launches behind the
    parameter gradients, which stay exactly what they are without it.
    plan (backward_plan): the gradients to form; every launch it does not need is skipped (frozen layers), and the gradients it
    forms are bit-identical to the all-trainable backward's.  None: every name in G, and the frames when dframes is given.
    dinter: upstream gradients of the intermediates() tensors (fp32 NCHW, same order, None where absent), added into the gradient
    slices where the reference graph has those tensors (nvq_inject_nchw); None or all-None: no launch."""
    if sv.feat0 is None:
        raise RuntimeError("forward(features=...) is an inference path: its result cannot be differentiated")
    g = sv.g
    if plan is None:
        plan = backward_plan(G.keys(), dframes is not None, g.NB, g.T)
    assert plan.frames == (dframes is not None), "backward: dframes and the plan disagree"
    x = _Bwd(P, sv, dout, G, plan, deterministic, dinter)
    # the transposed packs of the input-gradient convs outside the dense blocks in one launch (the blocks' mirror-form packs
    # have a batched launch of their own, _bwd_rdb); only the packs of the convs that run
    F, T, dxs, pre_a = g.F, g.T, plan.dx, "temporal_aggregator.attention."
    reqs = [r for st, r in (("up", ("upsampler.conv.weight", True, g.Up, F)), ("gff", ("gff.0.weight", True, F, F)),
                            ("att.4", (pre_a + "4.weight", True, g.Tp, F)), ("att.2", (pre_a + "2.weight", True, F, F)),
                            ("att.0", (pre_a + "0.weight", True, F, T * F))) if st in dxs]
    if g.NO:
        reqs += [(f"motion_estimator.flow_net.{idx}.weight", True, cs, keep)
                 for idx, cs, keep in zip((6, 4, 2, 0), (4, K.pad4(32), K.pad4(64), K.pad4(128)), (32, 64, 128, 81))
                 if f"flow.{idx}" in dxs]
    if reqs:
        x.packs.prefetch(reqs)
    # Frozen layers: a stage runs while something upstream of it, or one of its own parameters, needs a gradient (plan.run);
    # past the last such stage the pass ends.
    for stage in _BWD_STAGES:
        if not stage(x):
            break
    if x.small:
        x.wq.flush()
    x.G.check()
    if dframes is not None:
        # the head conv's input gradient for all T frames (same operands as its weight gradient), then the bicubic
        # skip's adjoint onto the centre frame, masked by the clamp
        wh = P["feature_extractor.head.0.weight"]
        if sv.img8 is not None:
            K.head_dgrad(x.dcur, wh, g.B, g.slots, dframes)
        else:
            K.head_dgrad(x.dcur, wh, g.B, g.slots, dframes, act=sv.feat0, dout2=x.dfeat_all)
        K.bicubic_adjoint(dout, sv.passmask, g.s, g.c, 1.0, dframes, accumulate=True)


# ----------------------------------------------------------------------------- LightweightSuperResolution
LIGHT_F = 32
LIGHT_BLOCKS = (2, 3, 4, 5)       # indices of the DepthwiseSeparableConv modules inside `net`

def light_forward(P: Dict[str, torch.Tensor], x: torch.Tensor, scale: int, training: bool, math: int = K.MATH_F32,
                  act_dtype: torch.dtype = torch.float32, sync: Optional[dict] = None) -> "tuple[torch.Tensor, Saved]":
    """Single-frame net (reference super_resolution.py:434-470): conv3x3+ReLU, four depthwise-separable blocks,
    conv3x3 -> PixelShuffle, + bicubic(x), clamp.  Same kernels as the SR feature extractor and tail.  sync: as in forward()."""
    assert act_dtype == torch.float32 or math == K.MATH_BF16
    dev = x.device
    B, Cimg, H, W = x.shape
    F = LIGHT_F
    frames = x.view(B, 1, Cimg, H, W)
    ws = workspace(dev)
    sv = Saved()
    sv.frames, sv.training, sv.math, sv.act_dtype, sv.scale = frames, training, math, act_dtype, scale
    feat0 = _new(dev, B, H, W, F, dtype=act_dtype)
    K.head_forward(frames, [0], P["net.0.weight"], P["net.0.bias"], feat0, math=math)
    sv.feat0, sv.dws, sv.pws, sv.acts, sv.bn_mean, sv.bn_invstd = feat0, [], [], [], [], []
    sv.bn_sync = []
    cur = feat0
    for k in LIGHT_BLOCKS:
        pre = f"net.{k}."
        d = _new(dev, B, H, W, F, dtype=act_dtype)
        K.dwconv_forward(cur, P[pre + "depthwise.weight"], d)
        p = _new(dev, B, H, W, F, dtype=act_dtype)
        K.conv_forward(Sl(d), K.conv_pack(P[pre + "pointwise.weight"], False, F, math=math), None, Sl(p), 1, math=math)
        mean, invstd = _new(dev, 1, F), _new(dev, 1, F)
        grp = sync.get(pre + "bn") if (training and sync) else None
        sv.bn_sync.append((grp, K.new_bn_stats(dev, 1, F)) if grp is not None else None)
        _bn_stats(P, pre + "bn.", p, B, [0], mean, invstd, ws, training, sv.bn_sync[-1])
        r = _new(dev, B, H, W, F, dtype=act_dtype)
        K.bn_apply_relu(p, B, mean, invstd, P[pre + "bn.weight"], P[pre + "bn.bias"], None, Sl(r), B)
        sv.dws.append(d); sv.pws.append(p); sv.acts.append(r); sv.bn_mean.append(mean); sv.bn_invstd.append(invstd)
        cur = r
    U = Cimg * scale * scale
    Up = K.pad4(U)
    out = _new(dev, B, Cimg, H * scale, W * scale)
    passmask = _new(dev, B, Cimg, H * scale, W * scale, dtype=torch.uint8)
    wup = K.conv_pack(P["net.6.weight"], False, F, math=math)
    if _fused_tail_ok(math, cur, Cimg, scale):
        K.upsampler_tail_forward(Sl(cur), wup, P["net.6.bias"], frames, 0, scale, out, passmask)
    else:
        u = _new(dev, B, H, W, Up)
        K.conv_forward(Sl(cur), wup, P["net.6.bias"], Sl(u, U), 3, cout_store=Up, math=math)
        K.shuffle_bicubic_clamp(u, frames, 0, scale, out, passmask)
    sv.passmask, sv.U, sv.Up = passmask, U, Up
    return out, sv


def light_backward(P: Dict[str, torch.Tensor], sv: Saved, dout: torch.Tensor, G: Dict[str, torch.Tensor],
                   dframes: Optional[torch.Tensor] = None, plan: Optional[BackwardPlan] = None) -> None:
    """dframes (B,1,3,H,W) fp32: also write the gradient w.r.t. the input image (overwrite).  plan (light_backward_plan): as in
    backward(); None: every name in G, and the image when dframes is given."""
    if plan is None:
        plan = light_backward_plan(G.keys(), dframes is not None)
    assert plan.frames == (dframes is not None), "light_backward: dframes and the plan disagree"
    run, dxs = plan.run, plan.dx
    G = _Grads(G, plan, P)
    dev = dout.device
    B, _, Cimg, H, W = sv.frames.shape
    F, math, act_dtype = LIGHT_F, sv.math, sv.act_dtype
    ws = workspace(dev)
    du = _new(dev, B, H, W, sv.Up)
    K.shuffle_clamp_backward(dout, sv.passmask, sv.scale, du)
    _wgrad(Sl(sv.acts[-1]), F, Sl(du, sv.U), G, "net.6.weight", "net.6.bias", ws, 3, math=math)
    dcur = None
    if "up" in dxs:
        dcur = _new(dev, B, H, W, F)
        K.conv_forward(Sl(du), K.conv_pack(P["net.6.weight"], True, sv.Up, F, math=math), None, Sl(dcur), 3, math=math)
    for j in range(len(LIGHT_BLOCKS) - 1, -1, -1):
        if f"block.{j}" not in run:             # (nor any block below it)
            break
        pre = f"net.{LIGHT_BLOCKS[j]}."
        dp = _bn_relu_bwd(P, G, pre, dcur, sv.pws[j], B, sv.bn_mean[j], sv.bn_invstd[j], sv.training, sv.bn_sync[j], ws)
        _wgrad(Sl(sv.dws[j]), F, Sl(dp), G, pre + "pointwise.weight", None, ws, 1, math=math)
        dww = G.get(pre + "depthwise.weight")
        if dww is None and f"block.{j}" not in dxs:
            break
        dd = torch.empty_like(dp)
        K.conv_forward(Sl(dp), K.conv_pack(P[pre + "pointwise.weight"], True, F, F, math=math), None, Sl(dd), 1, math=math)
        xin = sv.feat0 if j == 0 else sv.acts[j - 1]
        if dww is not None:
            K.dwconv_wgrad(xin, dd, dww, ws)
        if f"block.{j}" not in dxs:
            break
        dcur = torch.empty_like(dd, dtype=act_dtype if j > 0 else torch.float32)
        K.dwconv_forward(dd, P[pre + "depthwise.weight"], dcur, flip=True)
    hw = G.pair("net.0.weight", "net.0.bias") if "head" in run else None
    if hw is not None:
        K.head_wgrad(sv.frames, [0], dcur, sv.feat0, hw[0], hw[1] if hw[1] is not None else torch.empty_like(P["net.0.bias"]), ws)
    G.check()
    if dframes is not None:
        K.head_dgrad(dcur, P["net.0.weight"], B, [0], dframes, act=sv.feat0)
        K.bicubic_adjoint(dout, sv.passmask, sv.scale, 0, 1.0, dframes, accumulate=True)


def intermediates(sv: Saved) -> "list[torch.Tensor]":
    """return_intermediate payload in the reference's NCHW layout (super_resolution.py:384-389), fp32, in the order
    features[0 .. T-1], aligned[0 .. T-1], aggregated: one nvq_gather_nchw launch out of the NHWC slices."""
    g = sv.g
    B, T, F, c = g.B, g.T, g.F, g.c
    dev = sv.aligned.device
    outs = [_new(dev, B, F, g.H, g.W) for _ in range(2 * T + 1)]
    jobs = []
    for j, t in enumerate(g.slots):
        src = Sl(sv.aligned, F, c * F) if j == 0 else Sl(sv.feat_oth).images((j - 1) * B, j * B)
        jobs.append((src, outs[t]))
    jobs += [(Sl(sv.aligned, F, t * F), outs[T + t]) for t in range(T)]
    x0 = sv.xloc(0)
    jobs.append((Sl(x0.t, F, x0.coff), outs[2 * T]))
    K.gather_nchw(jobs)
    return outs
