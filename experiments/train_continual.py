#!/usr/bin/env python3
"""Continual-learning task sequence (BASELINE configs[4]): same CLI and loops as the reference's
experiments/train_continual.py (:15-145) on libnvq.

Declared deviation: the reference script crashes at its first ``ewc.register_task`` because
``EWC.compute_fisher`` feeds the 4-D loader batch to ``EnhancementEngine.forward`` (which needs 5-D input and
returns a dict).  Here EWC wraps a thin adapter around the same engine that maps (B,C,H,W) -> (B,3,C,H,W) and
returns ``['enhanced']``, so the Fisher / penalty actually run; everything up to that point prints what the
reference prints.  ``--tasks`` / ``--samples`` / ``--epochs`` are additions (defaults = the reference's values), and so are
``--precision`` / ``--graphs``: 64x64 clips are launch-bound on an MI355X, so the script runs the network
in its throughput mode by default - bf16 MFMA operands with fp32 accumulation and, for such small frames, HIP-graph replay of the
step (``net.use_hip_graphs = "auto"``); ``--precision fp32 --graphs off`` is the exact-fp32 parity mode the package defaults to.
``--device-memory`` (with ``--memory-storage`` / ``--prioritized``) keeps the replay memory in HBM (DeviceEpisodicMemory, DESIGN.md
section 16); without it the replay strategy runs the host-side EpisodicMemory and prints what it always printed.
``--strategy distill`` (with ``--distill-alpha`` / ``--feature-distill``) is the reference's fourth method, which its own script
imports and never runs: after every task the SR network is frozen into a teacher, and the next task's loss adds the fused
output and cosine feature distillation terms of csrc/distill.hip.
``--strategy agem`` (with ``--agem-ref-batch``; the memory flags of the replay strategy apply) is A-GEM: before every step the
gradient on a batch from the memory is taken as the reference, and a conflicting step gradient is projected onto its orthogonal
complement in place in the gradient bucket, decision included on the device (csrc/bucket_ops.hip).
``--strategy gem`` (with ``--gem-ref-batch`` / ``--gem-margin`` / ``--gem-eps`` / ``--gem-eps-relative`` / ``--gem-refresh``; the
memory flags apply) is GEM: one reference gradient per earlier task, drawn from the memory by content type, and the step gradient
is moved by the solution of a small quadratic program so that it opposes none of them (csrc/gem.hip).
``--clip-grad-norm X`` clips the global gradient norm before every optimizer step of any strategy with the same kernels.
``--drift {mmd,psi}`` (with ``--drift-grid G``) reports, before every task but the first, whether the task's LR frames have drifted
from the previous task's: nerve_cl.drift.DriftDetector on per-cell mean / deviation descriptors of the frames (csrc/drift.hip,
DESIGN.md section 22).  The script only reports; the task boundaries stay the ones it is given."""
import argparse
from pathlib import Path

import _common  # noqa: F401
import torch
import torch.nn as nn
from torch.utils.data import DataLoader, TensorDataset

from _common import (LOSS_CHOICES, add_optimizer_arguments, ema_weights, make_optimizer, optimizer_impl, pick_device, resolve_loss,
                     shard)
from nerve_cl import drift, metrics, ops, parallel
from nerve_cl.continual import AGEM, EWC, GEM, DeviceEpisodicMemory, EpisodicMemory, FOMAML, ContinualDistillation  # noqa: F401
from nerve_cl.models import EnhancementConfig, EnhancementEngine

OFFSETS = {"sports": 0.2, "animation": -0.2, "movie": 0.0, "news": 0.1}


def create_task_data(content_type: str, num_samples: int = 100):
    off = OFFSETS.get(content_type, 0)
    return torch.randn(num_samples, 3, 64, 64) + off, torch.randn(num_samples, 3, 128, 128) + off


class _ClipAdapter(nn.Module):
    """4-D frame batch -> engine -> 'enhanced' tensor; shares the engine's parameters."""

    def __init__(self, engine: EnhancementEngine):
        super().__init__()
        self.engine = engine

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        return self.engine(x.unsqueeze(1).expand(-1, 3, -1, -1, -1))["enhanced"]


class _SRClipAdapter(nn.Module):
    """4-D frame batch -> the engine's SR network on the repeated-frame clip, forwarding ``return_intermediate``: the student
    (and, deep-copied, the teacher) of the distill strategy.  enhancement_strength is 1 in this script, so the SR output is the
    engine's 'enhanced'.  Shares the engine's parameters."""

    def __init__(self, sr: nn.Module):
        super().__init__()
        self.sr = sr

    def forward(self, x: torch.Tensor, return_intermediate: bool = False):
        clip = x.unsqueeze(1).expand(-1, self.sr.num_frames, -1, -1, -1)
        return self.sr(clip, return_intermediate=True) if return_intermediate else self.sr(clip)


def configure_precision(model: EnhancementEngine, precision: str, graphs: str) -> None:
    """The script's precision / replay choice applied to the engine's SR network (knobs of nerve_cl.models.SuperResolutionNet,
    not part of the reference surface)."""
    from nerve_cl import _nvq
    sr = model.super_resolution
    sr.math_mode = _nvq.MATH_BF16 if precision == "bf16" else _nvq.MATH_F32
    sr.bf16_activations = precision == "bf16"
    sr.use_hip_graphs = {"auto": "auto", "on": True, "off": False}[graphs]


def make_criterion(config):
    """nn.MSELoss() of the reference as libnvq kernels, or the libnvq loss that --loss names"""
    name = config.get("loss", "mse")
    return ops.MSELoss() if name == "mse" else resolve_loss(name)


def build_optimizer(model, config):
    """Adam(lr=1e-4) of the reference through --optimizer-impl; the bucket form takes --clip-grad-norm as its max_grad_norm (the
    clip then costs no pass of its own and leaves .grad unscaled) and --ema-decay."""
    impl = config.get("optimizer_impl", "torch")
    kw = {}
    if impl == "bucket":
        kw = dict(max_grad_norm=config.get("clip_grad_norm"), ema_decay=config.get("ema_decay"), model=model)
    return make_optimizer(torch.optim.Adam, model.parameters(), impl, lr=1e-4, **kw)


def clip_gradients(model, config) -> None:
    """--clip-grad-norm: global 2-norm clipping on the gradient buckets, no host read (nothing without the flag, and nothing
    with --optimizer-impl bucket, whose update launch clips)"""
    max_norm = config.get("clip_grad_norm")
    if max_norm is not None and config.get("optimizer_impl", "torch") != "bucket":
        ops.clip_grad_norm_(model, max_norm)


def metrics_suffix(meter, world: int = 1) -> str:
    """' SSIM=... MAE=...' of the epoch's (detached) outputs against their targets; '' without --metrics"""
    if meter is None:
        return ""
    if world > 1:
        meter.all_reduce()
    m = meter.compute()
    return f" SSIM={m['ssim_global']:.4f} MAE={m['mae']:.4f}"


class DriftReport:
    """--drift: the descriptors of the last task's LR frames are the detector's reference; before the next task trains, its
    frames' descriptors are tested against them and one line is printed."""

    def __init__(self, method: str, grid: int, device):
        self.detector = drift.DriftDetector(method=method)
        self.grid, self.device = grid, device

    def __call__(self, task_id: int, lr: torch.Tensor, say) -> None:
        desc = drift.frame_descriptor(lr.to(self.device), grid=(self.grid, self.grid))
        if task_id > 0:
            r = self.detector.detect(desc)
            say(f"drift task {task_id - 1} -> {task_id}: method={r.method} score={r.score:.6f} drift={r.is_drift}")
        self.detector.set_reference(desc)


def report_drift(config, task_id: int, lr: torch.Tensor, say) -> None:
    """called when a task begins: nothing without --drift"""
    if config.get("drift") is not None:
        config["drift"](task_id, lr, say)


def train_with_ewc(model, tasks, config, rank=0, world=1, epochs=5, optimizer=None):
    device = next(model.parameters()).device
    adapter = _ClipAdapter(model)
    ewc = EWC(adapter, ewc_lambda=config.get("ewc_lambda", 5000))
    if optimizer is None:
        optimizer = build_optimizer(model, config)
    criterion = make_criterion(config)
    say = print if rank == 0 else (lambda *a, **k: None)
    for task_id, (task_name, (lr, hr)) in enumerate(tasks):
        report_drift(config, task_id, lr, say)
        say(f"\n=== Training on Task {task_id}: {task_name} ===")
        sl = shard(len(lr), rank, world)
        loader = DataLoader(TensorDataset(lr[sl], hr[sl]), batch_size=max(16 // world, 1), shuffle=True)
        for epoch in range(epochs):
            model.train()
            total = 0.0
            meter = metrics.QualityMeter() if config.get("metrics") else None
            for lr_b, hr_b in loader:
                lr_b, hr_b = lr_b.to(device), hr_b.to(device)
                optimizer.zero_grad()
                out = model(lr_b.unsqueeze(1).expand(-1, 3, -1, -1, -1))["enhanced"]
                loss = criterion(out, hr_b) + ewc.penalty()
                loss.backward()
                clip_gradients(model, config)
                optimizer.step()
                total += loss.item()
                if meter is not None:
                    meter.update(out, hr_b)
            if world > 1:                          # the printed loss is the mean over all ranks' batches (rank-uniform call)
                total = parallel.allreduce_scalars([total], device=device)[0] / world
            say(f"  Epoch {epoch + 1}: Loss={total / len(loader):.4f}{metrics_suffix(meter, world)}")
        ewc.register_task(task_id, loader)
        say(f"  Registered task {task_id} for EWC protection")
    return model


def train_with_replay(model, tasks, memory, config, rank=0, epochs=5, optimizer=None):
    device = next(model.parameters()).device
    if optimizer is None:
        optimizer = build_optimizer(model, config)
    criterion = make_criterion(config)
    on_device = isinstance(memory, DeviceEpisodicMemory)
    prioritized = bool(config.get("prioritized"))
    per_sample = resolve_loss(config.get("loss", "mse"))            # reduction="none": one value per sample
    say = print if rank == 0 else (lambda *a, **k: None)
    for task_id, (task_name, (lr, hr)) in enumerate(tasks):
        report_drift(config, task_id, lr, say)
        say(f"\n=== Training on Task {task_id}: {task_name} ===")
        for epoch in range(epochs):
            model.train()
            idx = torch.randperm(len(lr))[:16]
            lr_b, hr_b = lr[idx].to(device), hr[idx].to(device)
            n_cur, replayed = len(lr_b), None
            if len(memory) > 0:
                if on_device:                                       # one allocation, the replay rows gathered in place
                    lr_b, hr_b, replayed = memory.replay_batch(lr_b, hr_b, 8, weighted=prioritized)
                else:
                    r_lr, r_hr, _ = memory.sample(batch_size=8, device=device)
                    lr_b, hr_b = torch.cat([lr_b, r_lr]), torch.cat([hr_b, r_hr])
            optimizer.zero_grad()
            out = model(lr_b.unsqueeze(1).expand(-1, 3, -1, -1, -1))["enhanced"]
            if prioritized:
                values = per_sample(out, hr_b, reduction="none")
                loss = values.mean()
                if replayed is not None:                            # the replay rows' losses become their slots' importances
                    memory.update_importance(replayed, values.detach()[n_cur:], momentum=0.9)
            else:
                loss = criterion(out, hr_b)
            loss.backward()
            clip_gradients(model, config)
            optimizer.step()
            meter = None
            if config.get("metrics"):
                meter = metrics.QualityMeter()
                meter.update(out, hr_b)
            say(f"  Epoch {epoch + 1}: Loss={loss.item():.4f}{metrics_suffix(meter)}")
        store_task(memory, lr, hr, task_name)
        say(f"  Memory size: {len(memory)}")
    return model


def store_task(memory, lr, hr, task_name) -> None:
    """the first 50 samples of a finished task go to the memory (host or device class)"""
    n_store = min(50, len(lr))
    if isinstance(memory, DeviceEpisodicMemory):
        memory.store_batch(lr[:n_store], hr[:n_store], content_type=task_name)
    else:
        for i in range(n_store):
            memory.store(lr[i], hr[i], metadata={"content_type": task_name})


def train_with_agem(model, tasks, memory, config, rank=0, epochs=5, optimizer=None):
    """Shaped like train_with_replay: the memory's samples are not mixed into the batch, their gradient constrains the step's."""
    device = next(model.parameters()).device
    if optimizer is None:
        optimizer = build_optimizer(model, config)
    criterion = make_criterion(config)
    adapter = _ClipAdapter(model)
    agem = AGEM(adapter, memory, ref_batch_size=config.get("agem_ref_batch", 8))
    say = print if rank == 0 else (lambda *a, **k: None)
    for task_id, (task_name, (lr, hr)) in enumerate(tasks):
        report_drift(config, task_id, lr, say)
        say(f"\n=== Training on Task {task_id}: {task_name} ===")
        for epoch in range(epochs):
            model.train()
            idx = torch.randperm(len(lr))[:16]
            lr_b, hr_b = lr[idx].to(device), hr[idx].to(device)
            agem.compute_reference(criterion)                       # False (and no constraint) while the memory is empty
            optimizer.zero_grad()
            out = adapter(lr_b)
            loss = criterion(out, hr_b)
            loss.backward()
            agem.project()
            clip_gradients(model, config)
            optimizer.step()
            meter = None
            if config.get("metrics"):
                meter = metrics.QualityMeter()
                meter.update(out, hr_b)
            say(f"  Epoch {epoch + 1}: Loss={loss.item():.4f} cos(g,ref)={agem.cosine().item():+.4f}{metrics_suffix(meter)}")
        store_task(memory, lr, hr, task_name)
        say(f"  Memory size: {len(memory)}  projections so far: {agem.num_projections()}")
    return model


def train_with_gem(model, tasks, memory, config, rank=0, epochs=5, optimizer=None):
    """train_with_agem with one constraint per earlier task: every --gem-refresh-th step the references are taken again."""
    device = next(model.parameters()).device
    if optimizer is None:
        optimizer = build_optimizer(model, config)
    criterion = make_criterion(config)
    adapter = _ClipAdapter(model)
    gem = GEM(adapter, memory, ref_batch_size=config.get("gem_ref_batch", 8), margin=config.get("gem_margin", 0.5),
              eps=config.get("gem_eps", 1e-3), eps_relative=config.get("gem_eps_relative", False))
    refresh = max(int(config.get("gem_refresh", 1)), 1)
    say = print if rank == 0 else (lambda *a, **k: None)
    step = 0
    for task_id, (task_name, (lr, hr)) in enumerate(tasks):
        report_drift(config, task_id, lr, say)
        say(f"\n=== Training on Task {task_id}: {task_name} ===")
        for epoch in range(epochs):
            model.train()
            idx = torch.randperm(len(lr))[:16]
            lr_b, hr_b = lr[idx].to(device), hr[idx].to(device)
            if step % refresh == 0:
                gem.compute_references(criterion)                   # 0 rows (and no constraint) during the first task
            step += 1
            optimizer.zero_grad()
            out = adapter(lr_b)
            loss = criterion(out, hr_b)
            loss.backward()
            gem.project()
            clip_gradients(model, config)
            optimizer.step()
            meter = None
            if config.get("metrics"):
                meter = metrics.QualityMeter()
                meter.update(out, hr_b)
            st = gem.stats.tolist()                                 # one host read per printed line
            say(f"  Epoch {epoch + 1}: Loss={loss.item():.4f} min cos(g,r_t)={st[7]:+.4f} active={int(st[1])} |g|={st[5] ** 0.5:.3e}"
                f"{metrics_suffix(meter)}")
        store_task(memory, lr, hr, task_name)
        gem.add_task(task_name)
        say(f"  Memory size: {len(memory)}  projections so far: {gem.num_projections()}")
    return model


def train_with_distill(model, tasks, config, rank=0, epochs=5, optimizer=None):
    """Single process, unsharded.  With the MSE criterion the task term is folded into the distillation kernel (fold_task)."""
    device = next(model.parameters()).device
    distill = ContinualDistillation(_SRClipAdapter(model.super_resolution), alpha=config.get("distill_alpha", 0.5),
                                    feature_weight=config.get("feature_distill", 0.0),
                                    fold_task=config.get("loss", "mse") == "mse" and config.get("fold_task", True))
    if optimizer is None:
        optimizer = build_optimizer(model, config)
    criterion = make_criterion(config)
    say = print if rank == 0 else (lambda *a, **k: None)
    for task_id, (task_name, (lr, hr)) in enumerate(tasks):
        report_drift(config, task_id, lr, say)
        say(f"\n=== Training on Task {task_id}: {task_name} ===")
        loader = DataLoader(TensorDataset(lr, hr), batch_size=16, shuffle=True)
        for epoch in range(epochs):
            model.train()
            parts = torch.zeros(4, device=device)                   # total, task, distill, feature: one host read per epoch
            meter = metrics.QualityMeter() if config.get("metrics") else None
            for lr_b, hr_b in loader:
                lr_b, hr_b = lr_b.to(device), hr_b.to(device)
                optimizer.zero_grad()
                losses = distill.compute_loss(lr_b, hr_b, criterion)
                losses["total"].backward()
                clip_gradients(model, config)
                optimizer.step()
                feature = losses.get("feature", parts.new_zeros(()))
                parts += torch.stack([losses[k].detach().float() for k in ("total", "task", "distill")] + [feature.detach().float()])
                if meter is not None:
                    meter.update(distill.last_output, hr_b)
            total, task, dist, feat = (parts / len(loader)).tolist()
            say(f"  Epoch {epoch + 1}: Loss={total:.4f} Task={task:.4f} Distill={dist:.6f} Feature={feat:.6f}"
                f"{metrics_suffix(meter)}")
        distill.register_task()
        say(f"  Registered task {task_id} as the distillation teacher")
    return model


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser()
    ap.add_argument("--strategy", choices=["ewc", "replay", "maml", "distill", "agem", "gem"], default="ewc")
    ap.add_argument("--agem-ref-batch", type=int, default=8,
                    help="agem strategy: samples drawn from the memory for the reference gradient of every step")
    ap.add_argument("--gem-ref-batch", type=int, default=8,
                    help="gem strategy: samples drawn from the memory per earlier task for its reference gradient")
    ap.add_argument("--gem-margin", type=float, default=0.5,
                    help="gem strategy: lower bound of the multipliers (the published 'memory strength')")
    ap.add_argument("--gem-eps", type=float, default=1e-3, help="gem strategy: ridge added to the references' Gram matrix")
    ap.add_argument("--gem-eps-relative", action="store_true",
                    help="gem strategy: the ridge is --gem-eps times the largest squared reference norm")
    ap.add_argument("--gem-refresh", type=int, default=1, metavar="K",
                    help="gem strategy: take the reference gradients again every K-th step (1: every step, the published method)")
    ap.add_argument("--clip-grad-norm", type=float, default=None, metavar="X",
                    help="clip the global 2-norm of the gradient to X before every optimizer step (any strategy; default: no clipping)")
    ap.add_argument("--distill-alpha", type=float, default=0.5,
                    help="distill strategy: weight of the teacher term, alpha * mse(s, teacher) + (1 - alpha) * mse(s, target)")
    ap.add_argument("--feature-distill", type=float, default=0.0, metavar="W",
                    help="distill strategy: weight of the cosine feature distillation on the SR network's aggregated features "
                         "(0: output distillation only)")
    ap.add_argument("--memory-size", type=int, default=200)
    ap.add_argument("--ewc-lambda", type=float, default=5000)
    ap.add_argument("--tasks", type=int, default=4)
    ap.add_argument("--samples", type=int, default=200)
    ap.add_argument("--epochs", type=int, default=5)
    ap.add_argument("--features", type=int, default=64)
    ap.add_argument("--blocks", type=int, default=8)
    ap.add_argument("--precision", choices=["bf16", "fp32"], default="bf16",
                    help="MFMA operand precision of the convolutions (accumulation fp32; fp32 = the exact parity mode)")
    ap.add_argument("--graphs", choices=["auto", "on", "off"], default="auto",
                    help="HIP-graph replay of the training step (auto: for launch-bound frame sizes only)")
    ap.add_argument("--sync-bn", action="store_true",
                    help="synchronise BatchNorm statistics over the ranks (nn.SyncBatchNorm; only with a launcher such as torch.distributed.run, WORLD_SIZE > 1).  Steps with synchronised layers run eagerly: HIP-graph replay is off for them")
    ap.add_argument("--loss", choices=LOSS_CHOICES, default="mse",
                    help="data term of the training loss (libnvq kernels; default: the reference's MSE)")
    ap.add_argument("--metrics", action="store_true",
                    help="add the global-statistics SSIM and the MAE of each epoch's outputs to its progress line")
    ap.add_argument("--device-memory", action="store_true",
                    help="replay strategy: keep the memory in HBM (DeviceEpisodicMemory): batched stores, replay rows gathered behind the task batch by one launch")
    ap.add_argument("--memory-storage", choices=("fp32", "bf16"), default="fp32",
                    help="with --device-memory: element type of the stored samples (bf16 halves the footprint)")
    ap.add_argument("--prioritized", action="store_true",
                    help="with --device-memory: per-sample losses of the replay rows update their importances (momentum 0.9) and replay draws are weighted by them")
    ap.add_argument("--drift", choices=["off", "mmd", "psi"], default="off",
                    help="before every task but the first, test its LR frames' descriptors for drift against the previous task's and "
                         "print one line (RBF-kernel MMD or population stability index on the device; off: nothing)")
    ap.add_argument("--drift-grid", type=int, default=8, metavar="G",
                    help="with --drift: the frames are described by the mean and deviation of every cell of a G x G grid per channel")
    add_optimizer_arguments(ap, ema_note="write it to checkpoints/continual_model_ema.pt at the end (this script has no "
                                         "evaluation pass to run under it)")
    return ap


def main() -> None:
    ap = build_parser()
    args = ap.parse_args()
    if args.prioritized and not args.device_memory:
        ap.error("--prioritized needs --device-memory")
    if args.strategy == "maml" and (args.ema_decay is not None or args.optimizer_impl != "torch"):
        ap.error("--strategy maml trains nothing: --optimizer-impl / --ema-decay have no effect there")

    if args.strategy == "gem" and args.tasks - 1 > 15:
        ap.error("--strategy gem keeps at most 15 earlier tasks")

    device, rank, world = pick_device()
    torch.manual_seed(0)
    model = EnhancementEngine(EnhancementConfig(frame_recovery_enabled=False, super_resolution_enabled=True,
                                                sr_num_features=args.features,
                                                sr_num_residual_blocks=args.blocks)).to(device)
    configure_precision(model, args.precision, args.graphs)
    if world > 1:
        model = parallel.enable_data_parallel(model, sync_bn=args.sync_bn)
    tasks = [(ct, create_task_data(ct, args.samples)) for ct in list(OFFSETS)[:args.tasks]]
    config = {"ewc_lambda": args.ewc_lambda, "loss": args.loss, "metrics": args.metrics, "prioritized": args.prioritized,
              "distill_alpha": args.distill_alpha, "feature_distill": args.feature_distill,
              "agem_ref_batch": args.agem_ref_batch, "gem_ref_batch": args.gem_ref_batch, "gem_margin": args.gem_margin,
              "gem_eps": args.gem_eps, "gem_eps_relative": args.gem_eps_relative, "gem_refresh": args.gem_refresh,
              "clip_grad_norm": args.clip_grad_norm,
              "optimizer_impl": optimizer_impl(args), "ema_decay": args.ema_decay,
              "drift": DriftReport(args.drift, args.drift_grid, device) if args.drift != "off" else None}
    optimizer = build_optimizer(model, config)      # (the reference loops each build their own; the steps are the same)
    if args.strategy == "ewc":
        model = train_with_ewc(model, tasks, config, rank, world, args.epochs, optimizer=optimizer)
    elif args.strategy in ("replay", "agem", "gem"):
        if args.device_memory:
            memory = DeviceEpisodicMemory(capacity=args.memory_size, strategy="stratified", device=device,
                                          storage=args.memory_storage)
        else:
            memory = EpisodicMemory(capacity=args.memory_size, strategy="stratified")
        train = {"replay": train_with_replay, "agem": train_with_agem, "gem": train_with_gem}[args.strategy]
        model = train(model, tasks, memory, config, rank, args.epochs, optimizer=optimizer)
    elif args.strategy == "distill":
        if world > 1:
            ap.error("--strategy distill runs in a single process")
        model = train_with_distill(model, tasks, config, rank, args.epochs, optimizer=optimizer)
    # ('maml' has no branch in the reference either: it saves the untrained model)
    if rank == 0:
        Path("checkpoints").mkdir(exist_ok=True)
        torch.save(model.state_dict(), "checkpoints/continual_model.pt")
        if args.ema_decay is not None:                 # the weight average, for evaluation
            with ema_weights(optimizer):
                torch.save(model.state_dict(), "checkpoints/continual_model_ema.pt")
        print("\nTraining complete!")


if __name__ == "__main__":
    main()
