#!/usr/bin/env python3
"""Federated training in simulation mode: the reference's experiments/train_federated.py ``--mode simulation`` on libnvq, with the
rounds actually trained and aggregated (the reference's FederatedTrainer only counts samples).

Every client holds clips drawn around an offset of its own (the reference's create_client_data), shaped as train_continual.py
shapes its tasks.  A round trains the selected clients one after the other on the one model, whose flat parameter buffer is reset
to the global weights in place, and ends with one aggregation pass of csrc/federated.hip over the matrix of client weights
(nerve_cl.federated.FederatedTrainer).  ``--dp-enabled`` wraps the local optimizer in the per-tensor
clip-and-noise DPOptimizer (two launches on the gradient bucket); ``--update-clip`` / ``--update-noise`` / ``--server-lr`` act on
the clients' whole updates in the aggregation pass.  ``--clusters C`` (with ``--cluster-after R`` plain rounds first) is clustered
federated learning: one round clusters the clients by their updates (csrc/cluster.hip), every cluster then
has its own model; the sizes are printed after the split and every cluster's evaluation loss at the end.  ``--aggregator`` chooses
a Byzantine-robust rule instead of FedAvg (``median``, ``trimmed_mean`` with ``--trim-ratio``, ``krum`` / ``multi_krum`` with
``--num-byzantine``; csrc/robust.hip), and ``--poison N`` makes the first N selected clients of every round
hostile through the trainer's ``after_client`` hook: ``--poison-kind flip`` sends ``global - 10 (x - global)``, ``nan`` sends NaN
weights.  With either option the evaluation loss of the global model over all clients' data is printed after every round: FedAvg
breaks under ``--poison 1``, the robust rules hold.  ``--server-opt`` runs a FedOpt server optimizer on the aggregated update
(``fedavgm``, ``fedadagrad``, ``fedadam``, ``fedyogi`` with ``--server-beta1`` / ``--server-beta2`` / ``--server-tau``; ``--server-lr``
is its learning rate, and 1.0 is far too large for the adaptive ones) and ``--prox-mu`` adds FedProx's proximal term to the local
steps (csrc/fedopt.hip); ``--eval`` prints the evaluation loss after every round.  ``--compress`` compresses
every client's update before the aggregation (csrc/compress.hip): ``topk`` keeps the ``--compress-ratio``
largest coordinates, ``quant`` quantises to ``--compress-levels`` levels (QSGD), ``topk_quant`` does both; what is not sent stays in
the client's residual for the next round unless ``--no-error-feedback``.  Every round then prints the mean kept share and the
modelled bytes sent as a fraction of dense fp32 (``wire_bytes``: a model, nothing is serialised).  The ``server`` and ``client``
modes need the flwr transport and exit saying so.
"""
import argparse
from pathlib import Path

import _common  # noqa: F401
import torch

from _common import OPTIMIZER_IMPLS, pick_device
from nerve_cl import ops
from nerve_cl.federated import COMPRESSIONS, SERVER_OPTIMIZERS, FederatedTrainer, PrivacyConfig, wire_bytes
from nerve_cl.federated.trainer import AGGREGATORS
from nerve_cl.models import EnhancementConfig, EnhancementEngine
from train_continual import _ClipAdapter, configure_precision


def create_client_data(client_id: int, num_samples: int = 100):
    """heterogeneous clients: every client's frames sit around an offset of its own, (client_id % 5) * 0.1 as in the reference"""
    off = (client_id % 5) * 0.1
    return torch.randn(num_samples, 3, 64, 64) + off, torch.randn(num_samples, 3, 128, 128) + off


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["simulation", "server", "client"], default="simulation")
    ap.add_argument("--num-clients", type=int, default=10)
    ap.add_argument("--clients-per-round", type=int, default=5)
    ap.add_argument("--num-rounds", type=int, default=10)
    ap.add_argument("--local-epochs", type=int, default=5)
    ap.add_argument("--dp-enabled", action="store_true", help="per-tensor gradient clipping and Gaussian noise in every local step")
    ap.add_argument("--dp-noise-multiplier", type=float, default=1.0)
    ap.add_argument("--dp-max-grad-norm", type=float, default=1.0)
    ap.add_argument("--update-clip", type=float, default=None, metavar="X",
                    help="clip every client's whole update to the 2-norm X in the aggregation pass (default: no clipping)")
    ap.add_argument("--update-noise", type=float, default=0.0, metavar="S",
                    help="standard deviation of the Gaussian noise added to the aggregated weights")
    ap.add_argument("--server-lr", type=float, default=1.0,
                    help="the aggregated update is scaled by this before it is applied; with --server-opt the server optimizer's "
                         "learning rate.  BEWARE: fedadagrad / fedadam / fedyogi move every weight by about this much per round, so "
                         "the default 1.0 (a FedAvg value) is far too large for them: try 1e-3 .. 1e-1")
    ap.add_argument("--server-opt", choices=SERVER_OPTIMIZERS, default=None,
                    help="FedOpt: treat the aggregated update as a pseudo-gradient of server momentum (fedavgm), Adagrad, Adam or "
                         "Yogi (no --clusters); see the warning at --server-lr")
    ap.add_argument("--server-beta1", type=float, default=0.9, help="--server-opt: momentum")
    ap.add_argument("--server-beta2", type=float, default=0.99, help="--server-opt fedadam / fedyogi: second-moment decay")
    ap.add_argument("--server-tau", type=float, default=1e-3, help="--server-opt: adaptivity, the floor of the denominator")
    ap.add_argument("--prox-mu", type=float, default=0.0, metavar="MU",
                    help="FedProx: add MU / 2 |theta - theta_round|^2 to every client's objective (default 0: off)")
    ap.add_argument("--compress", choices=COMPRESSIONS, default=None,
                    help="compress every client's update before the aggregation: top-k sparsification, QSGD quantisation or both "
                         "(no --clusters)")
    ap.add_argument("--compress-ratio", type=float, default=0.01, metavar="R", help="--compress topk*: the share of coordinates kept")
    ap.add_argument("--compress-levels", type=int, default=127, metavar="S", help="--compress *quant: quantisation levels, 1 .. 32767")
    ap.add_argument("--no-error-feedback", action="store_true",
                    help="--compress: drop what a client did not send instead of adding it to its next update")
    ap.add_argument("--clusters", type=int, default=1, metavar="C",
                    help="cluster the clients by their updates into C groups with one model each (default 1: plain FedAvg)")
    ap.add_argument("--cluster-after", type=int, default=0, metavar="R", help="plain FedAvg rounds before the round that clusters")
    ap.add_argument("--aggregator", choices=AGGREGATORS, default="fedavg",
                    help="how a round combines the clients' weights: FedAvg, or a Byzantine-robust rule (no --update-clip, no --clusters)")
    ap.add_argument("--trim-ratio", type=float, default=0.1,
                    help="trimmed_mean: the share of the clients dropped from each side of every coordinate")
    ap.add_argument("--num-byzantine", type=int, default=0, metavar="F", help="krum / multi_krum: the number of clients assumed hostile")
    ap.add_argument("--poison", type=int, default=0, metavar="N", help="the first N selected clients of every round send poisoned weights")
    ap.add_argument("--poison-kind", choices=["flip", "nan"], default="flip",
                    help="flip: global - 10 (x - global), the sign-flipped, scaled update; nan: NaN weights")
    ap.add_argument("--eval", action="store_true", help="print the evaluation loss of the global model after every round")
    ap.add_argument("--samples", type=int, default=100, help="clips per client (the reference's 100)")
    ap.add_argument("--features", type=int, default=64)
    ap.add_argument("--blocks", type=int, default=8)
    ap.add_argument("--precision", choices=["bf16", "fp32"], default="bf16",
                    help="MFMA operand precision of the convolutions (accumulation fp32; fp32 = the exact parity mode)")
    ap.add_argument("--optimizer-impl", choices=OPTIMIZER_IMPLS, default="torch",
                    help="torch: torch.optim's fused AdamW (default); bucket: nerve_cl.optim.BucketAdamW on the flat buckets")
    ap.add_argument("--seed", type=int, default=0, help="client selection, data and every noise stream")
    return ap


def evaluate(trainer) -> float:
    """the mean loss of the model as it stands over every client's data"""
    model, loss = trainer.model, ops.MSELoss()
    was_training = model.training
    model.eval()
    total, seen = 0.0, 0
    with torch.no_grad():
        for xs, ys in trainer.client_data.values():
            for i in range(0, len(xs), trainer.batch_size):
                x, y = xs[i:i + trainer.batch_size], ys[i:i + trainer.batch_size]
                total += float(loss(model(x), y)) * len(x)
                seen += len(x)
    model.train(was_training)
    return total / max(seen, 1)


def main() -> None:
    ap = build_parser()
    args = ap.parse_args()
    if args.mode != "simulation":
        raise SystemExit(f"--mode {args.mode} needs the `flwr` transport, which this package does not wrap; "
                         "--mode simulation runs the same rounds in one process")
    device, rank, world = pick_device()
    if world > 1:
        ap.error("the federated simulation runs in a single process")
    torch.manual_seed(args.seed)
    engine = EnhancementEngine(EnhancementConfig(frame_recovery_enabled=False, super_resolution_enabled=True,
                                                 sr_num_features=args.features, sr_num_residual_blocks=args.blocks)).to(device)
    configure_precision(engine, args.precision, "off")
    privacy = None
    if args.dp_enabled:
        privacy = PrivacyConfig(max_grad_norm=args.dp_max_grad_norm, noise_multiplier=args.dp_noise_multiplier)
    poison = {"left": 0, "global": None}               # armed before every round: the clients still to poison, the global weights

    def after_client(client_id, model):
        if poison["left"] <= 0:
            return
        poison["left"] -= 1
        for v, g in zip(model.state_dict().values(), poison["global"]):
            if v.is_floating_point():
                v.copy_(torch.full_like(v, float("nan")) if args.poison_kind == "nan" else g - 10.0 * (v - g))

    trainer = FederatedTrainer(_ClipAdapter(engine), num_clients=args.num_clients, clients_per_round=args.clients_per_round,
                               local_epochs=args.local_epochs, loss=ops.MSELoss(), privacy=privacy, update_clip=args.update_clip,
                               update_noise=args.update_noise, server_lr=args.server_lr, optimizer_impl=args.optimizer_impl,
                               seed=args.seed, num_clusters=args.clusters, cluster_after=args.cluster_after,
                               aggregator=args.aggregator, trim_ratio=args.trim_ratio, num_byzantine=args.num_byzantine,
                               after_client=after_client if args.poison > 0 else None, server_optimizer=args.server_opt,
                               server_betas=(args.server_beta1, args.server_beta2), server_tau=args.server_tau,
                               prox_mu=args.prox_mu, compression=args.compress, compress_ratio=args.compress_ratio,
                               compress_levels=args.compress_levels, error_feedback=not args.no_error_feedback)
    for cid in range(args.num_clients):
        lr, hr = create_client_data(cid, args.samples)
        trainer.set_client_data(cid, (lr.to(device), hr.to(device)))          # on the device: a round copies nothing from the host
    for _ in range(args.num_rounds):
        if args.poison > 0:
            poison["left"] = args.poison
            poison["global"] = [v.detach().clone() for v in trainer.model.state_dict().values()]
        m = trainer.train_round()
        print(f"Round {m['round']}: {m['clients']} clients, {m['samples']} samples, loss {m['train_loss']:.4f}")
        if args.eval or args.poison > 0 or args.aggregator != "fedavg":
            chosen = f", selected {[int(w) for w in m['selected_weights']]}" if "selected_weights" in m else ""
            print(f"  evaluation loss of the global model {evaluate(trainer):.4f}{chosen}")
        if "kept" in m:
            levels = args.compress_levels if args.compress.endswith("quant") else 0
            sizes = [r.shape[1] for r in trainer._plan["rows"]] or [trainer._plan["n_params"]]
            share = sum(sum(ks) / (len(ks) * n) for ks, n in zip(m["kept"], sizes)) / len(sizes)
            sent = sum(wire_bytes(n, k, levels) for ks, n in zip(m["kept"], sizes) for k in ks)
            dense = sum(4 * n * len(ks) for ks, n in zip(m["kept"], sizes))
            print(f"  compressed updates: kept {share:.4f} of the coordinates, modelled {sent / dense:.4f} of the dense bytes")
        if args.clusters > 1 and m["round"] == args.cluster_after + 1:
            print(f"  clusters after the split: sizes {m['clusters']}, clients {trainer.client_cluster}")
    if trainer.cluster_models is not None:
        model, loss = trainer.model, ops.MSELoss()
        for c in range(args.clusters):
            members = [cid for cid, k in trainer.client_cluster.items() if k == c]
            if not members:
                print(f"Cluster {c}: empty")
                continue
            trainer.load_cluster(c)
            model.eval()
            total, seen = 0.0, 0
            with torch.no_grad():
                for cid in members:
                    xs, ys = trainer.client_data[cid]
                    for i in range(0, len(xs), trainer.batch_size):
                        x, y = xs[i:i + trainer.batch_size], ys[i:i + trainer.batch_size]
                        total += float(loss(model(x), y)) * len(x)
                        seen += len(x)
            print(f"Cluster {c}: {len(members)} clients, eval loss {total / max(seen, 1):.4f}")
        trainer.load_mean()
    Path("checkpoints").mkdir(exist_ok=True)
    torch.save(engine.state_dict(), "checkpoints/federated_model.pt")
    print("\nFederated training complete!")


if __name__ == "__main__":
    main()
