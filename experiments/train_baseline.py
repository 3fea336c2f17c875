#!/usr/bin/env python3
"""Baseline SR training (BASELINE configs[0]): same CLI, model arguments, optimiser, loss, PSNR formula,
T=3 `expand` trick, progress line and best-checkpoint rule as the reference's
experiments/train_baseline.py (:35-147), running on libnvq.  Launch with torch.distributed.run for
data-parallel training (each rank trains on its shard; gradients are all-reduced inside backward)."""
import argparse
import copy
import time
from pathlib import Path

import _common  # noqa: F401  (sys.path)
import torch
import torch.nn as nn
from torch.utils.data import DataLoader, TensorDataset

from _common import (LOSS_CHOICES, add_optimizer_arguments, compute_psnr, ema_weights, make_optimizer, optimizer_impl, pick_device,
                     resolve_loss, shard)
from nerve_cl import metrics, ops, parallel
from nerve_cl.models import SuperResolutionNet


def load_split(data_dir: str, split: str, rank: int, world: int) -> TensorDataset:
    blob = torch.load(f"{data_dir}/{split}/data.pt")
    sl = shard(len(blob["lr"]), rank, world)
    return TensorDataset(blob["lr"][sl], blob["hr"][sl])


def as_clip(lr: torch.Tensor) -> torch.Tensor:
    return lr.unsqueeze(1).expand(-1, 3, -1, -1, -1)      # (B,3,C,H,W), stride-0 like the reference (:82)


def train(args) -> None:
    device, rank, world = pick_device()
    say = print if rank == 0 else (lambda *a, **k: None)
    say(f"Using device: {device}")
    say("Loading dataset...")
    train_set, val_set = load_split(args.data_dir, "train", rank, world), load_split(args.data_dir, "val", rank, world)
    say(f"  Train samples: {len(train_set)}")
    say(f"  Val samples: {len(val_set)}")
    train_loader = DataLoader(train_set, batch_size=args.batch_size, shuffle=True)
    val_loader = DataLoader(val_set, batch_size=args.batch_size)

    say("Creating model...")
    model = SuperResolutionNet(scale_factor=2, num_features=32, num_residual_blocks=4, temporal_window=1).to(device)
    if world > 1:
        model = parallel.enable_data_parallel(model, sync_bn=args.sync_bn)
    say(f"  Parameters: {sum(p.numel() for p in model.parameters()):,}")
    impl = optimizer_impl(args)
    extra_kw = dict(ema_decay=args.ema_decay, model=model) if impl == "bucket" else {}
    optimizer = make_optimizer(torch.optim.AdamW, model.parameters(), impl, lr=args.lr, weight_decay=1e-5, **extra_kw)
    scheduler = torch.optim.lr_scheduler.CosineAnnealingLR(optimizer, T_max=args.epochs)
    # nn.MSELoss() of the reference, as libnvq kernels; --loss picks another libnvq loss
    criterion = ops.MSELoss() if args.loss == "mse" else resolve_loss(args.loss)

    say(f"\nTraining for {args.epochs} epochs...")
    say("-" * 60)
    best_psnr, t_start = 0, time.time()
    for epoch in range(args.epochs):
        model.train()
        running = 0.0
        for lr, hr in train_loader:
            lr, hr = lr.to(device), hr.to(device)
            optimizer.zero_grad()
            loss = criterion(model(as_clip(lr)), hr)
            loss.backward()
            optimizer.step()
            running += loss.item()
        running /= max(len(train_loader), 1)

        model.eval()
        val_loss = val_psnr = 0.0
        meter = metrics.QualityMeter() if args.metrics else None
        with torch.no_grad(), ema_weights(optimizer):       # --ema-decay: validate the weight average
            for lr, hr in val_loader:
                lr, hr = lr.to(device), hr.to(device)
                out = model(as_clip(lr))
                val_loss += criterion(out, hr).item()
                val_psnr += compute_psnr(out, hr)
                if meter is not None:
                    meter.update(out, hr)       # device-side sums, no host synchronisation
        # rank-uniform validation numbers (each rank validated its shard): every rank must take the same branch below,
        # because the branch contains collectives
        val_loss, val_psnr, nval = parallel.allreduce_scalars([val_loss, val_psnr, len(val_loader)], device=device)
        val_loss /= max(nval, 1)
        val_psnr /= max(nval, 1)
        scheduler.step()
        extra = ""
        if meter is not None and nval > 0:
            meter.all_reduce()
            m = meter.compute()
            extra = f"Val SSIM: {m['ssim_global']:.4f} | Val MAE: {m['mae']:.4f} | "
        say(f"Epoch {epoch + 1:3d}/{args.epochs} | Train Loss: {running:.4f} | Val Loss: {val_loss:.4f} | "
            f"Val PSNR: {val_psnr:.2f} dB | {extra}Time: {time.time() - t_start:.1f}s")
        if val_psnr > best_psnr:
            best_psnr = val_psnr
            if world > 1:
                parallel.average_bn_buffers_(model)
            if rank == 0:
                model_state = model.state_dict()
                if args.ema_decay is not None:              # the checkpoint holds the weights that were validated
                    with ema_weights(optimizer):
                        model_state = copy.deepcopy(model_state)
                torch.save({"epoch": epoch, "model_state_dict": model_state,
                            "optimizer_state_dict": optimizer.state_dict(), "psnr": best_psnr},
                           "checkpoints/best_model.pt")
    say("-" * 60)
    say("Training complete!")
    say(f"  Best PSNR: {best_psnr:.2f} dB")
    say(f"  Total time: {time.time() - t_start:.1f}s")
    say("  Model saved: checkpoints/best_model.pt")


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description="Train NERVE baseline")
    ap.add_argument("--data-dir", type=str, default="data")
    ap.add_argument("--batch-size", type=int, default=16)
    ap.add_argument("--epochs", type=int, default=10)
    ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("--sync-bn", action="store_true",
                    help="synchronise BatchNorm statistics over the ranks (nn.SyncBatchNorm; only with a launcher such as torch.distributed.run, WORLD_SIZE > 1).  Steps with synchronised layers run eagerly: HIP-graph replay is off for them")
    ap.add_argument("--loss", choices=LOSS_CHOICES, default="mse",
                    help="training and validation loss (libnvq kernels; default: the reference's MSE)")
    ap.add_argument("--metrics", action="store_true",
                    help="add the global-statistics SSIM and the MAE of the validation set to the progress line")
    add_optimizer_arguments(ap)
    return ap


def main() -> None:
    args = build_parser().parse_args()
    Path("checkpoints").mkdir(exist_ok=True)
    train(args)


if __name__ == "__main__":
    main()
