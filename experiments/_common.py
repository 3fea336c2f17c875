"""Shared bits of the experiment scripts: path setup, PSNR, optional one-process-per-GPU launch."""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "continual-learning-for-dynamic-video-quality-enhancement_amd")
if PKG not in sys.path:
    sys.path.insert(0, PKG)

import torch  # noqa: E402


def compute_psnr(pred: torch.Tensor, target: torch.Tensor) -> float:
    """20*log10(1/sqrt(mse)) over the whole batch (reference experiments/train_baseline.py:27-32)."""
    mse = torch.mean((pred - target) ** 2)
    if mse == 0:
        return float("inf")
    return 20 * torch.log10(1.0 / torch.sqrt(mse)).item()


LOSS_CHOICES = ("mse", "l1", "charbonnier", "ssim", "ms_ssim", "ms_ssim_l1")


def resolve_loss(name: str):
    """The libnvq loss f(pred, target, reduction="mean") that --loss names.  The multi-scale ones take as many scales as the
    target frame allows (ops.ms_ssim_max_scales: 4 at 128 x 128) with the standard weights renormalised."""
    from nerve_cl import ops
    if name in ops.LOSSES:
        return ops.LOSSES[name]
    fn = {"ms_ssim": ops.ms_ssim_loss, "ms_ssim_l1": ops.ms_ssim_l1_loss}[name]

    def loss(pred, target, reduction="mean"):
        weights = ops.ms_ssim_weights(ops.ms_ssim_max_scales(*target.shape[-2:]))
        return fn(pred, target, weights=weights, reduction=reduction)
    return loss


def pick_device():
    """'cuda' when a HIP device is visible (reference train_baseline.py:37); the SR path has no CPU mode."""
    from nerve_cl import parallel
    rank, world, local = parallel.init_from_env()
    if not torch.cuda.is_available():
        raise SystemExit("no HIP device visible: nerve_cl's super-resolution path runs only on the GPU")
    torch.cuda.set_device(local)
    return torch.device("cuda", local), rank, world


OPTIMIZER_IMPLS = ("torch", "bucket")


def make_optimizer(cls, params, impl: str = "torch", **kw):
    """The reference's `torch.optim.Adam / AdamW(model.parameters(), ...)` call (train_continual.py:27,51, train_baseline.py:41).

    impl "torch" (the default): PyTorch's fused single-kernel implementation when every parameter is an fp32 tensor on the GPU:
    the same update rule; the default (foreach) form is ~10 launches and 0.6 ms of host time per step over the network's 131
    tensors, which the launch-bound 64x64 steps feel.

    impl "bucket": nerve_cl.optim.BucketAdam / BucketAdamW for Adam / AdamW - the same rule as one libnvq launch per run of
    parameters on the flat buckets; takes max_grad_norm= / ema_decay= / model= on top of torch's arguments."""
    if impl == "bucket":
        from nerve_cl import optim
        bucket = {torch.optim.Adam: optim.BucketAdam, torch.optim.AdamW: optim.BucketAdamW}.get(cls)
        if bucket is None:
            raise NotImplementedError(f"--optimizer-impl bucket: no flat-bucket form of {cls.__name__} (Adam and AdamW only)")
        return bucket(params, **kw)
    if impl != "torch":
        raise ValueError(f"optimizer impl {impl!r}: one of {OPTIMIZER_IMPLS}")
    params = list(params)
    if params and all(p.is_cuda and p.dtype == torch.float32 for p in params):
        kw.setdefault("fused", True)
    return cls(params, **kw)


def add_optimizer_arguments(ap, ema_note: str = "evaluate / save with it") -> None:
    """--optimizer-impl / --ema-decay of the training scripts; ema_note: what the script does with the average"""
    ap.add_argument("--optimizer-impl", choices=OPTIMIZER_IMPLS, default="torch",
                    help="torch: torch.optim's fused Adam (default); bucket: nerve_cl.optim on the flat parameter / gradient "
                         "buckets, one launch per step")
    ap.add_argument("--ema-decay", type=float, default=None, metavar="D",
                    help="keep an exponential moving average of the weights with decay D inside the optimizer launch and "
                         f"{ema_note} (implies --optimizer-impl bucket)")


def optimizer_impl(args) -> str:
    return "bucket" if getattr(args, "ema_decay", None) is not None else getattr(args, "optimizer_impl", "torch")


def ema_weights(optimizer):
    """Context for an evaluation pass: the optimizer's weight average in place of the weights (nothing without --ema-decay)"""
    import contextlib
    if getattr(optimizer, "ema_decay", None) is not None:
        return optimizer.swap_ema()
    return contextlib.nullcontext()


def shard(n: int, rank: int, world: int) -> slice:
    """Contiguous shard of a dataset of n samples for this rank.  Every rank gets the SAME number of samples (the
    remainder n % world is dropped): the gradient all-reduce runs once per training batch inside backward, so ranks with
    different batch counts would wait for each other forever."""
    per = n // world
    return slice(rank * per, (rank + 1) * per)
