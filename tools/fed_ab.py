"""Bit identity of the federated aggregation across two checkouts: print one `case sha256` line per case of a fixed list, so
that two runs (each a fresh process) agree exactly when their outputs are identical files.
usage: python tools/fed_ab.py --tree <checkout root> > hashes.txt
The package directory of that checkout goes on sys.path and NVQ_LIB points at its libnvq.so.  Cases: aggregate_flat,
aggregate_flat_clustered (C = 1, 3, 8; no base, a shared base, one base per cluster), aggregate_flat_trimmed (trim 0, 1, median) and
krum_aggregate_flat for K in 1, 3, 9, 17, 33, 64 and n in 3, 5, 1023, the matrix 16-byte aligned and shifted by one float, with and
without base, clip and noise as far as the function takes them; one n = 1024 * 1024 + 1031 case each at K = 3 (a second trip of
the grid); then two rounds of FederatedTrainer on a small SR network per aggregator, hashing the model's state.
usage: python tools/fed_ab.py --fedopt [--iters 20] [--rounds 5] [--no-training] [--out profiles/fedopt.txt]
Another job on this tool's own checkout: time the FedOpt server rules and the FedProx gradient (see fedopt_profile)."""
import argparse
import hashlib
import itertools
import os
import sys

PKG = "continual-learning-for-dynamic-video-quality-enhancement_amd"


def digest(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().cpu().contiguous().numpy().tobytes())
    return h.hexdigest()


def fedopt_profile(args):
    """--fedopt: time nvq_fed_server_opt and nvq_fed_prox_grad (csrc/fedopt.hip) on the default SR network's
    flat buffer and write profiles/fedopt.txt in the format of profiles/robust_aggregation.txt (tools/robust_probe.py).
      (a) nvq_fed_aggregate, the yardstick: 4 n (K + 2) bytes;
      (b) nvq_fed_server_opt per rule: 4 n (K + 4) bytes for fedavgm (base and m read, out and m written), 4 n (K + 6) with v;
      (c) what a user composes without it: nvq_fed_aggregate into a vector, then the server step in torch operations; its rate
          is against the bytes of (b), what the job has to move.
    Then nvq_fed_prox_grad against g.add_(theta - anchor, alpha=mu) (16 n bytes), the time of a FederatedTrainer round with and
    without the two options, and (unless --no-training) the evaluation loss after experiments/train_federated.py's default rounds
    for fedavg, every server rule at three server learning rates, and --prox-mu 0.01."""
    import subprocess

    import torch

    tools = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, tools)
    from robust_probe import LINES, alternate, row, say
    from nerve_cl import _nvq
    from nerve_cl.federated import SERVER_OPTIMIZERS, FederatedTrainer
    from nerve_cl.models import SuperResolutionNet

    assert torch.cuda.is_available(), "the probe times the MI355X"
    dev = torch.device("cuda", 0)
    net = SuperResolutionNet().to(dev)
    n = net._bucket_layout()[1]
    lr, b1, b2, tau, mu = 1e-2, 0.9, 0.99, 1e-3, 0.01
    say(f"flat parameter buffer of the default SR network: {n} floats ({4 * n / 1e6:.1f} MB); {args.iters} calls per timing, "
        f"{args.rounds} alternated rounds (us per call)")

    def torch_step(rule, agg, base, m, v, out):
        D = agg - base
        if rule == "fedavgm":
            m.mul_(b1).add_(D)
            return torch.add(base, m, alpha=lr, out=out)
        m.mul_(b1).add_(D, alpha=1 - b1)
        if rule == "fedadagrad":
            v.addcmul_(D, D)
        elif rule == "fedadam":
            v.mul_(b2).addcmul_(D, D, value=1 - b2)
        else:
            d2 = D * D
            v.sub_(torch.sign(v - d2).mul_(d2), alpha=1 - b2)
        return torch.addcdiv(base, m, v.sqrt().add_(tau), value=lr, out=out)

    for K in (5, 10, 64):
        torch.manual_seed(K)
        base = net.flat_theta().clone()
        clients = base.repeat(K, 1) + 1e-3 * torch.randn(K, n, device=dev)
        w = torch.arange(1, K + 1, dtype=torch.float64, device=dev)
        out, agg, ref = (torch.empty(n, device=dev) for _ in range(3))

        def k_aggregate():
            _nvq.fed_aggregate(clients, n, base, w, None, out)

        ta = alternate((k_aggregate,), args.iters, args.rounds)[0]
        best_a = row(f"K = {K:2d} (a) nvq_fed_aggregate", ta, 4 * n * (K + 2))
        for rule in SERVER_OPTIMIZERS:
            rid = SERVER_OPTIMIZERS.index(rule)
            m, mt = torch.zeros(n, device=dev), torch.zeros(n, device=dev)
            v, vt = torch.full((n,), tau * tau, device=dev), torch.full((n,), tau * tau, device=dev)

            def k_opt():
                _nvq.fed_server_opt(clients, n, base, w, None, rid, m, v, out, server_lr=lr, beta1=b1, beta2=b2, tau=tau)

            def t_opt():
                _nvq.fed_aggregate(clients, n, base, w, None, agg)
                torch_step(rule, agg, base, mt, vt, ref)

            k_opt(), t_opt()
            say(f"K = {K}: {rule}, kernel against nvq_fed_aggregate + the fp32 torch composition: max difference "
                f"{(out - ref).abs().max().item():.1e} (max |theta| {base.abs().max().item():.2f})")
            nb = 4 * n * (K + (4 if rule == "fedavgm" else 6))
            tk, tt = alternate((k_opt, t_opt), args.iters, args.rounds)
            bk = row(f"K = {K:2d} (b) {rule}: nvq_fed_server_opt", tk, nb)
            bt = row(f"K = {K:2d} (c) {rule}: nvq_fed_aggregate + torch", tt, nb)
            say(f"  {'':52s} (c) / (b) {bt / bk:.2f}x   (b) / (a) {bk / best_a:.2f}x, the traffic ratio is {nb / (4 * n * (K + 2)):.2f}x")

    torch.manual_seed(1)
    theta, anchor = net.flat_theta().clone(), net.flat_theta().clone() + 1e-3 * torch.randn(n, device=dev)
    g, gt = torch.randn(n, device=dev), torch.randn(n, device=dev)
    tk, tt = alternate((lambda: _nvq.fed_prox_grad(g, theta, anchor, mu), lambda: gt.add_(theta - anchor, alpha=mu)), args.iters,
                       args.rounds)
    bk = row("nvq_fed_prox_grad", tk, 16 * n)
    bt = row("g.add_(theta - anchor, alpha=mu)", tt, 16 * n)
    say(f"  {'':52s} torch / kernel {bt / bk:.2f}x")

    # a round of the trainer: 5 clients x 8 clips of 3 frames 32 x 32, one local epoch in batches of 4, host clock, synchronised
    import time
    options = {"fedavg": {}, "fedadam": dict(server_optimizer="fedadam", server_lr=1e-3), "prox_mu 0.01": dict(prox_mu=0.01),
               "fedadam + prox_mu 0.01": dict(server_optimizer="fedadam", server_lr=1e-3, prox_mu=0.01)}
    trainers = {}
    for name, kw in options.items():
        torch.manual_seed(3)
        tr = FederatedTrainer(SuperResolutionNet().to(dev).train(), num_clients=5, clients_per_round=5, local_epochs=1, lr=1e-4,
                              batch_size=4, seed=8, **kw)
        for c in range(5):
            gen = torch.Generator().manual_seed(20 + c)
            tr.set_client_data(c, (torch.rand(8, 3, 3, 32, 32, generator=gen).to(dev), torch.rand(8, 3, 64, 64, generator=gen).to(dev)))
        tr.train_round()
        trainers[name] = tr
    times = {name: [] for name in options}
    for _ in range(args.rounds):
        for name, tr in trainers.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            tr.train_round_device()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) * 1e3)
    say(f"one FederatedTrainer round, default SR network, 5 clients x 2 local steps, {args.rounds} alternated rounds (ms per round)")
    for name, ts in times.items():
        say(f"  {name:52s} {' '.join(f'{t:8.2f}' for t in ts)}   best {min(ts):8.2f} ms")

    def flush():
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write("\n".join(LINES) + "\n")

    flush()
    if args.no_training:
        return
    # the script's default rounds on its seeded client data; the server learning rates of the sweep are fixed here, not tuned further
    script = os.path.join(tools, "..", "experiments", "train_federated.py")
    sweep = {"fedavgm": (0.1, 0.3, 1.0), "fedadagrad": (1e-3, 1e-2, 1e-1), "fedadam": (1e-3, 1e-2, 1e-1), "fedyogi": (1e-3, 1e-2, 1e-1)}
    runs = [("fedavg", []), ("fedavg --prox-mu 0.01", ["--prox-mu", "0.01"])]
    for i in (1, 0, 2):                                # every rule at its middle rate first: a budget that runs out leaves no rule out
        runs += [(f"{rule} --server-lr {lrs[i]:g}", ["--server-opt", rule, "--server-lr", f"{lrs[i]:g}"]) for rule, lrs in sweep.items()]
    say("evaluation loss of the global model over all clients' data after experiments/train_federated.py's default rounds (--eval, "
        "--seed 0); server learning rates swept: " + "; ".join(f"{r} {lrs}" for r, lrs in sweep.items()))
    began = time.perf_counter()
    for name, extra in runs:
        if time.perf_counter() - began > args.training_budget:
            say(f"  {name:40s} not run: the budget of {args.training_budget:g} s for these runs was used up")
            continue
        try:
            r = subprocess.run([sys.executable, script, "--eval"] + extra + args.script_args.split(), capture_output=True,
                               text=True, cwd=args.workdir, timeout=args.script_timeout)
        except subprocess.TimeoutExpired:
            say(f"  {name:40s} ended after {args.script_timeout:g} s; no further run is started")
            flush()
            return
        losses = [ln.split("global model")[1].split()[0].rstrip(",") for ln in r.stdout.splitlines() if "evaluation loss" in ln]
        say(f"  {name:40s} " + (f"first round {losses[0]}   last round {losses[-1]}" if r.returncode == 0 and losses
                                else f"failed (exit {r.returncode}): {r.stderr.strip().splitlines()[-1:]}"))
        flush()
        if r.returncode != 0:                          # whatever it was, nothing further is started on the device
            return


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    ap.add_argument("--fedopt", action="store_true", help="time the FedOpt / FedProx kernels and write profiles/fedopt.txt instead")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "fedopt.txt"))
    ap.add_argument("--no-training", action="store_true", help="--fedopt: leave out the runs of experiments/train_federated.py")
    ap.add_argument("--script-args", default="", help="--fedopt: further arguments of every run of the script")
    ap.add_argument("--script-timeout", type=float, default=600.0, help="--fedopt: seconds after which a run of the script is ended")
    ap.add_argument("--training-budget", type=float, default=3600.0, help="--fedopt: start no further run of the script after this many seconds")
    ap.add_argument("--workdir", default=None, help="--fedopt: where the script runs (it writes checkpoints/ there)")
    args = ap.parse_args()
    tree = os.path.abspath(args.tree)
    os.environ["NVQ_LIB"] = os.path.join(tree, PKG, "libnvq.so")
    sys.path.insert(0, os.path.join(tree, PKG))
    if args.fedopt:
        return fedopt_profile(args)
    import torch
    from nerve_cl import federated as fed
    from nerve_cl.models import SuperResolutionNet

    assert torch.cuda.is_available(), "the comparison is of the device kernels"
    dev = torch.device("cuda", 0)

    def matrix(K, n, shift):
        """K rows of n floats, the row stride a multiple of 4, the first row 16-byte aligned or one float behind that"""
        stride = (n + 3) // 4 * 4 + 4
        g = torch.Generator().manual_seed(1000 * K + n)
        flat = torch.randn(K * stride + 4, generator=g).to(dev)
        return flat[shift:shift + K * stride].view(K, stride)[:, :n], torch.randn(n, generator=g).to(dev)

    def cases(K, n, shifts=(0, 1), small=True):
        opts = list(itertools.product((False, True), repeat=3)) if small else [(True, True, True), (True, False, True)]
        for shift, (has_base, clip, noise) in itertools.product(shifts, opts):
            clients, base = matrix(K, n, shift)
            tag = f"K{K} n{n} shift{shift} base{int(has_base)} clip{int(clip)} noise{int(noise)}"
            kw = dict(server_lr=0.5, noise_std=0.25 if noise else 0.0, seed=11, offset=4)
            b = base if has_base else None
            w = [float(k + 1) for k in range(K)]
            yield f"flat {tag}", lambda: fed.aggregate_flat(clients, w, base=b, clip_norm=2.0 if clip else None, **kw)
            for C, per in itertools.product((1, 3, 8), (False, True)):
                if per and (clip or not has_base):                     # a clip needs one shared base
                    continue
                labels = [(3 * k + 1) % (C + 1) - 1 for k in range(K)]  # -1 (left out) and every cluster that K reaches
                bases = base.repeat(C, 1) + torch.arange(C, device=dev).view(C, 1) if per else b
                yield (f"clustered C{C} per{int(per)} {tag}",
                       lambda: fed.aggregate_flat_clustered(clients, w, labels, C, bases=bases, clip_norm=2.0 if clip else None, **kw))
            if clip:                                                    # the robust rules take no clip
                continue
            for trim in (0, 1, fed.robust.TRIM_MEDIAN):
                yield f"trimmed t{trim} {tag}", lambda: fed.aggregate_flat_trimmed(clients, trim, base=b, **kw)
            if K >= 3:
                f = 0 if K < 5 else 1
                yield f"krum f{f} {tag}", lambda: fed.krum_aggregate_flat(clients, f, max(1, K // 2), base=b, **kw)

    for K, n in itertools.product((1, 3, 9, 17, 33, 64), (3, 5, 1023)):
        for name, fn in cases(K, n):
            print(name, digest(fn()), flush=True)
    for name, fn in cases(3, 1024 * 1024 + 1031, shifts=(0,), small=False):
        print(name, digest(fn()), flush=True)

    for agg in fed.trainer.AGGREGATORS:
        torch.manual_seed(3)
        net = SuperResolutionNet(num_features=16, num_residual_blocks=1).to(dev).train()
        net.deterministic = True
        tr = fed.FederatedTrainer(net, num_clients=4, clients_per_round=4, local_epochs=1, lr=1e-3, batch_size=4, seed=8,
                                  update_clip=1.0 if agg == "fedavg" else None, update_noise=1e-4, server_lr=0.5, aggregator=agg)
        for c in range(4):
            g = torch.Generator().manual_seed(20 + c)
            tr.set_client_data(c, (torch.rand(8, 3, 3, 16, 16, generator=g).to(dev), torch.rand(8, 3, 32, 32, generator=g).to(dev)))
        for _ in range(2):
            tr.train_round()
        print(f"trainer {agg}", digest(*net.state_dict().values()), flush=True)


if __name__ == "__main__":
    main()
