"""Shared by tests/test_optim_cpu.py and tests/test_optim_gpu.py: the float64 Adam / AdamW recurrence and the derived rounding bound;
and, run as a script, the rank body of test_optim_gpu.py::test_two_ranks_stay_bit_identical (launched with torch.distributed.run,
2 ranks sharing the one GPU of the box over gloo, as tests/agem_worker.py): enable_data_parallel -> three
BucketAdamW(max_grad_norm, ema_decay) steps on this rank's shard.

The bound.  After K steps, elementwise,

    |theta - theta_f64| <= K * (2^-22 * max(|theta_0|, |theta_f64|) + 2^-16 * lr)

against the same recurrence in float64, and the same form with lr -> 1, relative, for the rest:

    v:   K * (2^-22 * max(|v_0|, |v_f64|) + 2^-16 * |v_f64|)                    (a sum of non-negative terms: nothing cancels)
    m:   K * (2^-22 * max(|m_0|, |m_f64|) + 2^-23 * max_k |g_k|)
    EMA: theta's bound + K * 2^-23 * max(|ema_0|, |ema_f64|)

m is the one departure: it is a signed sum and cancels to zero in some elements, where a bound relative to |m| fails in any
precision (torch's own fp32 Adam exceeds it on the issue's inputs).  Its additive term is what the rounding supports instead.
With g the effective gradient (clipped, with the L2 term) and G = max_k |g_k|, one step rounds g (at most three roundings,
3 * 2^-24 G), g - m (2^-24 * 2 G), both scaled by 1 - beta1 = 0.1, and the fma (2^-24 |m| <= 2^-24 G): below 1.6 * 2^-24 G, asserted
at 2^-23 G per step.  The EMA is a convex combination of the thetas plus one subtraction and one fma per step, hence
tighter than the relative form."""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (REPO, os.path.join(REPO, "continual-learning-for-dynamic-video-quality-enhancement_amd"), os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402


class AdamF64:
    """torch.optim.Adam / AdamW (amsgrad=False, maximize=False) in float64 on one flat tensor, with the optional clipping
    coefficient and weight EMA of nvq_adam_step"""

    def __init__(self, theta, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, decoupled=False, ema_decay=None, m=None, v=None,
                 ema=None, step=0):
        self.theta0 = theta.detach().double().cpu().reshape(-1).clone()
        self.theta = self.theta0.clone()
        self.m = torch.zeros_like(self.theta) if m is None else m.detach().double().cpu().reshape(-1).clone()
        self.v = torch.zeros_like(self.theta) if v is None else v.detach().double().cpu().reshape(-1).clone()
        self.m0, self.v0 = self.m.clone(), self.v.clone()
        self.ema = (self.theta.clone() if ema is None else ema.detach().double().cpu().reshape(-1).clone()) if ema_decay is not None else None
        self.ema0 = None if self.ema is None else self.ema.clone()
        self.lr, self.betas, self.eps, self.wd, self.decoupled, self.ema_decay = lr, betas, eps, weight_decay, decoupled, ema_decay
        self.t, self.steps = step, 0
        self.gmax = torch.zeros_like(self.theta)          # max_k |effective g_k|

    def step(self, grad, lr=None, max_norm=None, total_norm=None):
        """total_norm (with max_norm): the global norm of the whole step's gradients, of which `grad` may be one part"""
        lr = self.lr if lr is None else lr
        b1, b2 = self.betas
        g = grad.detach().double().cpu().reshape(-1)
        if max_norm is not None:
            norm = float(g.norm()) if total_norm is None else float(total_norm)
            coef = max_norm / (norm + 1e-6)
            if coef < 1.0:
                g = g * coef
        if self.decoupled:
            self.theta = self.theta * (1.0 - lr * self.wd)
        else:
            g = g + self.wd * self.theta
        self.gmax = torch.maximum(self.gmax, g.abs())
        self.t += 1
        self.steps += 1
        self.m = self.m + (g - self.m) * (1.0 - b1)
        self.v = b2 * self.v + (1.0 - b2) * g * g
        bias1, bias2_sqrt = 1.0 - b1 ** self.t, (1.0 - b2 ** self.t) ** 0.5
        self.theta = self.theta - (lr / bias1) * self.m / (self.v.sqrt() / bias2_sqrt + self.eps)
        if self.ema is not None:
            self.ema = self.ema_decay * self.ema + (1.0 - self.ema_decay) * self.theta
        self.lr_max = max(getattr(self, "lr_max", 0.0), lr)

    # ------------------------------------------------------------------ the bounds after self.steps steps
    def theta_bound(self):
        return self.steps * (2.0 ** -22 * torch.maximum(self.theta0.abs(), self.theta.abs()) + 2.0 ** -16 * self.lr_max)

    def m_bound(self):
        return self.steps * (2.0 ** -22 * torch.maximum(self.m0.abs(), self.m.abs()) + 2.0 ** -23 * self.gmax)

    def v_bound(self):
        return self.steps * (2.0 ** -22 * torch.maximum(self.v0.abs(), self.v.abs()) + 2.0 ** -16 * self.v.abs())

    def ema_bound(self):
        return self.theta_bound() + self.steps * 2.0 ** -23 * torch.maximum(self.ema0.abs(), self.ema.abs())

    def check(self, theta, m=None, v=None, ema=None, what=""):
        """assert every element within its bound; prints the largest share of the bound first (pytest -s)"""
        for name, got, want, bound in (("theta", theta, self.theta, self.theta_bound()), ("m", m, self.m, self.m_bound()),
                                       ("v", v, self.v, self.v_bound()),
                                       ("ema", ema, self.ema, self.ema_bound() if self.ema is not None else None)):
            if got is None:
                continue
            err, bound = (got.detach().double().cpu().reshape(-1) - want.reshape(-1)).abs(), bound.reshape(-1)
            share = (err / bound.clamp_min(1e-300)).max().item() if err.numel() else 0.0      # (a zero bound asks for err == 0)
            print(f"{what} {name}: largest error / bound = {share:.4f}")
            assert bool((err <= bound).all()), (what, name, share)


def theta_bound_against(theta0, got, ref, steps, lr):
    """the theta bound with another implementation's result `ref` in the place of theta_f64 (class tests against torch.optim)"""
    a, b, c = (t.detach().double().cpu().reshape(-1) for t in (theta0, got, ref))
    bound = steps * (2.0 ** -22 * torch.maximum(a.abs(), c.abs()) + 2.0 ** -16 * lr)
    return ((b - c).abs() / bound).max().item()


# ------------------------------------------------------------------------------------------------- two ranks
CFG = dict(scale_factor=2, sr_num_features=16, sr_num_residual_blocks=1, sr_temporal_window=1)
B_PER_RANK, H, W = 2, 16, 24


def make_engine():
    from nerve_cl.models import EnhancementConfig, EnhancementEngine
    from oracle import synth
    eng = EnhancementEngine(EnhancementConfig(frame_recovery_enabled=False, **CFG))
    eng.super_resolution.load_state_dict(synth.formula_state(3, 2, 16, 1, 1, gain=synth.GOLDEN_GAIN))
    return eng


def data(world: int):
    from oracle import synth
    n = B_PER_RANK * world
    return synth.formula_clip(n, 3, H, W), synth.formula_target(n, 2 * H, 2 * W)


def main():
    import torch.nn.functional as F
    out_path = sys.argv[1]
    from nerve_cl import parallel
    from nerve_cl.optim import BucketAdamW
    rank, world, local = parallel.init_from_env("gloo")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    eng = make_engine().to(dev)
    if rank == 1:                                   # replicas start different; enable_data_parallel must fix that
        with torch.no_grad():
            for p in eng.parameters():
                p.mul_(1.5)
    parallel.enable_data_parallel(eng)
    x, y = data(world)
    mine = slice(B_PER_RANK * rank, B_PER_RANK * (rank + 1))
    xs, ys = x[mine].to(dev), y[mine].to(dev)
    opt = BucketAdamW(eng.parameters(), lr=1e-3, max_grad_norm=1e-3, ema_decay=0.9, model=eng)
    eng.train()
    launches = []
    for _ in range(3):
        opt.zero_grad()
        F.mse_loss(eng(xs)["enhanced"], ys).backward()      # the bucket hook leaves the rank mean: the same gradient on both ranks
        opt.step()
        launches.append(opt.last_launches)
    theta = eng.super_resolution.flat_theta().detach().cpu()
    ema = opt._nets[0].ema.detach().cpu()
    norm = opt.last_grad_norm.cpu()
    gathered = [torch.empty_like(theta) for _ in range(world)]
    torch.distributed.all_gather(gathered, theta)
    emas = [torch.empty_like(ema) for _ in range(world)]
    torch.distributed.all_gather(emas, ema)
    norms = [torch.empty_like(norm) for _ in range(world)]
    torch.distributed.all_gather(norms, norm)
    # a loose parameter that carries a gradient is refused under max_grad_norm: nothing synchronises it over the ranks
    eng.enhancement_strength.grad = torch.ones_like(eng.enhancement_strength)
    try:
        opt.step()
        refused = False
    except RuntimeError as e:
        refused = "enhancement_strength" in str(e)
    assert refused
    if rank == 0:
        torch.save({"theta": gathered, "ema": emas, "norm": norms, "launches": launches}, out_path)
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
