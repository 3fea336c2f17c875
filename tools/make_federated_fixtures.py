#!/usr/bin/env python3
"""Record tests/golden/federated_privacy.npz from the reference implementation's nerve_cl/federated/privacy.py.

    python tools/make_federated_fixtures.py --reference /path/to/reference/checkout

Only that one file is loaded, by path (the reference package's __init__ imports flwr).  Recorded, as data only:
  * compute_noise_multiplier and get_privacy_spent at a handful of arguments;
  * for a small seeded torch model and noise_multiplier = 0: the initial weights, the batch, and every parameter's gradient before
    and after the reference DPOptimizer.step() clips it (inner optimizer: plain SGD), plus the weights after the step.
Runs on the CPU; not part of the test suite."""
import argparse
import importlib.util
import os

import numpy as np
import torch
import torch.nn as nn

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NOISE_ARGS = [(8.0, 1e-5, 0.01, 1), (8.0, 1e-5, 0.1, 5), (1.0, 1e-6, 0.05, 3), (3.5, 1e-4, 0.25, 10), (0.5, 1e-5, 1.0, 2)]
SPENT_ARGS = [(100, 1.0, 0.01, 1e-5), (1, 0.5, 0.1, 1e-5), (5000, 1.1, 0.02, 1e-6), (37, 4.0, 0.25, 1e-4), (1000, 0.3, 1.0, 1e-5)]
MAX_GRAD_NORM, BATCH, SGD_LR = 0.2, 6, 0.1


def small_model() -> nn.Module:
    """what the tests rebuild: the weights come from the fixture, so only the shapes matter"""
    return nn.Sequential(nn.Conv2d(3, 5, 3, padding=1), nn.ReLU(), nn.Conv2d(5, 3, 3, padding=1, bias=False), nn.Flatten(),
                         nn.Linear(3 * 6 * 6, 7))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="checkout of the reference implementation")
    ap.add_argument("--out", default=os.path.join(REPO, "tests", "golden", "federated_privacy.npz"))
    args = ap.parse_args()
    spec = importlib.util.spec_from_file_location("reference_privacy",
                                                  os.path.join(args.reference, "nerve_cl", "federated", "privacy.py"))
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)

    out = {"noise_args": np.array(NOISE_ARGS, dtype=np.float64),
           "noise_values": np.array([ref.compute_noise_multiplier(e, d, q, int(n)) for e, d, q, n in NOISE_ARGS], dtype=np.float64),
           "spent_args": np.array(SPENT_ARGS, dtype=np.float64),
           "spent_values": np.array([ref.get_privacy_spent(int(s), m, q, d) for s, m, q, d in SPENT_ARGS], dtype=np.float64),
           "max_grad_norm": np.float64(MAX_GRAD_NORM), "batch_size": np.int64(BATCH), "sgd_lr": np.float64(SGD_LR)}
    torch.manual_seed(1234)
    model = small_model()
    x, y = torch.randn(BATCH, 3, 6, 6), torch.randn(BATCH, 7)
    out["x"], out["y"] = x.numpy(), y.numpy()
    names = [n for n, _ in model.named_parameters()]
    out["names"] = np.array(names)
    for n, p in model.named_parameters():
        out["w0/" + n] = p.detach().numpy().copy()
    cfg = ref.PrivacyConfig(max_grad_norm=MAX_GRAD_NORM, noise_multiplier=0.0)
    dp = ref.DPOptimizer(torch.optim.SGD(model.parameters(), lr=SGD_LR), model, cfg, BATCH, 60)
    dp.zero_grad()
    nn.functional.mse_loss(model(x), y).backward()
    for n, p in model.named_parameters():
        out["g/" + n] = p.grad.detach().numpy().copy()
    grads = [p.grad for p in model.parameters()]
    dp.step()
    for (n, p), g in zip(model.named_parameters(), grads):
        out["clipped/" + n] = g.detach().numpy().copy()
        out["w1/" + n] = p.detach().numpy().copy()
    norms = [float(np.linalg.norm(out["g/" + n].astype(np.float64))) for n in names]
    assert min(norms) < MAX_GRAD_NORM < max(norms), f"the bound should split the tensors: {norms}"
    np.savez_compressed(args.out, **out)
    print(f"wrote {args.out}: {os.path.getsize(args.out)} bytes, gradient norms {['%.4f' % v for v in norms]}")


if __name__ == "__main__":
    main()
