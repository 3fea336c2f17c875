"""GPU: csrc/abr.hip (vectorised streaming environment, fused act, GAE, PPO loss) and the PPOAgent's device rollout against the
float64 yardstick of tests/_abr_oracle.py.

Bounds.
  Environment: the device runs the oracle's float64 operations in the oracle's order; observations to 1 fp32 ulp, rewards to 1e-12
  relative, flags equal.  Asserted on the oracle alone first: no battery value in (0, 1e-9) and no buffer level within 1e-9 of 0
  before clamping, so no flag or clamp hangs on the last bit (seed 0 passes; a seed that did not would be replaced here).
  With max_steps = 12 an episode ends before the battery can run out (12 steps cost at most 0.36), so that case shows step-count
  termination and the same-step reset; battery truncation is shown by the same rollout with max_steps = 36, where row 0 (always
  enhancement 4, 0.03 per step) truncates at its 34th step.
  Act: head outputs, log-probability and value against the float64 oracle within 8 x the error of torch's CPU fp32 forward of the
  same network on the same inputs (floor 1e-6 max|ref|): the fp32 MFMA adds in another order than the CPU GEMM, both are fp32
  accurate.  Actions: the oracle's inverse CDF on the DEVICE's head outputs with the host Philox uniforms; a sample whose u lies
  within 1e-5 of a CDF boundary is left out, at most 1 % may be.
  GAE: every element within 1e-6 relative plus the absolute floor of _gae_floor (the cancellation in delta; fp32 scan).  PPO loss: loss, statistics and gradient within 8 x the error of the
  same composition evaluated by torch in fp32 on the CPU; the inputs keep every ratio 1e-4 away from 1 +- clip (asserted).
  Measured values of these errors are recorded in profiles/abr.txt."""
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import _abr_oracle as O  # noqa: E402

GOLDEN = os.path.join(HERE, "golden", "abr_reference.npz")


def _dev():
    return torch.device("cuda", 0)


def _ulps(a, b):
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


# ---------------------------------------------------------------------------------------------------------------- environment
N_ENV, T_ENV, SEED_ENV = 70, 40, 0
_env_cache = {}


def _env_case(max_steps):
    """(actions (T, N, 2), oracle rollout), computed once per max_steps and left unchanged"""
    if max_steps not in _env_cache:
        rng = np.random.default_rng(1234)
        actions = rng.integers(0, 5, size=(T_ENV, N_ENV, 2))
        actions[:, 0, 1] = 4
        checks = []
        ref = O.vec_rollout(N_ENV, actions, SEED_ENV, max_steps, checks=checks)
        level = np.array([c[0] for c in checks])
        battery = np.array([c[1] for c in checks])
        assert not ((battery > 0) & (battery < 1e-9)).any(), "precondition: a battery value in (0, 1e-9); choose another seed"
        assert not (np.abs(level) < 1e-9).any(), "precondition: a buffer level within 1e-9 of 0; choose another seed"
        _env_cache[max_steps] = (actions, ref)
    return _env_cache[max_steps]


@pytest.mark.parametrize("max_steps", [12, 36])
def test_env_matches_oracle(max_steps):
    from nerve_cl.abr import VecStreamingEnv
    actions, ref = _env_case(max_steps)
    done = ref["terminated"] | ref["truncated"]
    if max_steps == 12:
        assert ref["terminated"].any() and done[:-1].any(), "step-count termination and a same-step reset must occur"
    else:
        assert ref["truncated"][33, 0] and not ref["terminated"][33, 0] and ref["terminated"].any(), "both kinds must occur"
    env = VecStreamingEnv(N_ENV, max_steps=max_steps, seed=SEED_ENV, device=_dev())
    assert env.state.dtype == torch.float64 and env.counters.dtype == torch.int64
    obs0 = env.obs.cpu().numpy()
    assert _ulps(obs0, ref["obs0"]).max() <= 1
    a_dev = torch.as_tensor(actions, dtype=torch.int32).to(_dev())
    outs = [env.step(a_dev[t]) for t in range(T_ENV)]
    worst_ulp = max(int(_ulps(o[0].cpu().numpy(), ref["obs"][t]).max()) for t, o in enumerate(outs))
    worst_rew = max(float(np.abs(o[1].cpu().numpy() - ref["reward"][t]).max()) for t, o in enumerate(outs))
    print(f"env max_steps={max_steps}: observations differ by at most {worst_ulp} ulp, rewards by at most {worst_rew:.3e}")
    for t, (obs, reward, term, trunc, info) in enumerate(outs):
        assert obs.dtype == torch.float32 and reward.dtype == torch.float64 and term.dtype == torch.bool
        assert np.array_equal(term.cpu().numpy(), ref["terminated"][t]), t
        assert np.array_equal(trunc.cpu().numpy(), ref["truncated"][t]), t
        assert _ulps(obs.cpu().numpy(), ref["obs"][t]).max() <= 1, t
        r = reward.cpu().numpy()
        assert (np.abs(r - ref["reward"][t]) <= 1e-12 * np.abs(ref["reward"][t])).all(), t
        for k in ("vmaf", "rebuffer", "bandwidth", "buffer", "episode_return"):
            v = info[k].cpu().numpy()
            assert (np.abs(v - ref[k][t]) <= 1e-12 * np.abs(ref[k][t])).all(), (t, k)
    # the same-step reset: where an episode ended the returned observation is the next episode's first one
    t, e = np.argwhere(done)[0]
    o = outs[t][0][e].cpu().numpy()
    assert o[6] == 0.0 and o[2] == 1.0 and o[3] == np.float32(2 / 5)
    assert (env.counters.cpu().numpy() == T_ENV + 1).all()
    fin = env.finished.cpu().numpy()
    assert np.array_equal(fin[:, 1], done.sum(axis=0))
    assert np.allclose(fin[:, 0], (ref["episode_return"] * done).sum(axis=0), rtol=1e-12)


# ---------------------------------------------------------------------------------------------------------------- act
# "wide": every other path of the kernel at once: whole-float4 first-layer loads (obs_dim 32), three layers, the 512-wide layer's
# 68 KB of LDS, four heads, and 25 head outputs (the second 16-column head tile)
NETS = {"default": (7, (5, 5), (256, 256)), "uneven": (7, (3, 7), (64, 32)), "unsupported": (7, (5, 5), (48, 48)),
        "wide": (32, (6, 5, 4, 9), (512, 96, 32))}
_net_cache = {}


def _net(name):
    """(module on the device, float64 state, obs (1000, 7)), built once"""
    from nerve_cl.abr import ActorCritic
    if name not in _net_cache:
        obs_dim, heads, hidden = NETS[name]
        torch.manual_seed(5)
        net = ActorCritic(obs_dim, heads, hidden)
        with torch.no_grad():
            for h in net.policy_heads:          # spread the logits so that the CDFs are not all near uniform
                h.weight.mul_(8.0)
        sd = {k: v.clone() for k, v in net.state_dict().items()}
        obs = torch.rand(1000, obs_dim, generator=torch.Generator().manual_seed(9))
        _net_cache[name] = (net.to(_dev()), {k: v.double().numpy() for k, v in sd.items()}, obs, sd)
    return _net_cache[name]


def _bound(ref, fp32):
    return max(8.0 * np.abs(fp32 - ref).max(), 1e-6 * np.abs(ref).max())


@pytest.mark.parametrize("B", [1, 33, 70])
@pytest.mark.parametrize("name", list(NETS))
def test_act_matches_oracle(name, B):
    from nerve_cl.abr import ActorCritic
    obs_dim, heads, hidden = NETS[name]
    net, state, obs_all, sd = _net(name)
    assert net.fused == (name != "unsupported")
    obs = obs_all[:B]
    counters = torch.arange(B, dtype=torch.int64) * 3 + 7
    seed = 21
    a, lp, v, x = net.act(obs.to(_dev()), counters.to(_dev()), seed=seed, return_head_outputs=True)
    assert a.dtype == torch.int32 and tuple(a.shape) == (B, len(heads)) and tuple(lp.shape) == (B,) and tuple(v.shape) == (B,)
    a, lp, v, x = a.cpu().numpy(), lp.cpu().numpy().astype(np.float64), v.cpu().numpy().astype(np.float64), x.cpu().numpy()
    ref = O.mlp(state, obs.numpy(), len(hidden), len(heads))
    cpu = ActorCritic(obs_dim, heads, hidden)
    cpu.load_state_dict(sd)
    with torch.no_grad():
        x_cpu = torch.cat(cpu(obs), dim=-1)
    tol = _bound(ref, x_cpu.numpy().astype(np.float64))
    err = np.abs(x - ref).max()
    print(f"act {name} B={B}: head outputs err {err:.3e}, torch CPU fp32 err {np.abs(x_cpu.numpy() - ref).max():.3e}, bound {tol:.3e}")
    assert err <= tol
    assert np.abs(v - ref[:, -1]).max() <= tol
    ref_lp = O.log_prob_of(ref, heads, a)
    off, lp_cpu = 0, 0
    for j, n in enumerate(heads):
        lp_cpu = lp_cpu + torch.log_softmax(x_cpu[:, off:off + n], -1).gather(1, torch.as_tensor(a[:, j:j + 1], dtype=torch.int64))[:, 0]
        off += n
    tol_lp = _bound(ref_lp, lp_cpu.numpy().astype(np.float64))
    print(f"    log-prob err {np.abs(lp - ref_lp).max():.3e}, torch CPU fp32 err {np.abs(lp_cpu.numpy() - ref_lp).max():.3e}")
    assert np.abs(lp - ref_lp).max() <= tol_lp
    u = np.array([O.uniforms(seed, e, int(counters[e]), 1)[:len(heads)] for e in range(B)])
    want, _, margin = O.sample(x, heads, u)
    keep = margin >= 1e-5
    assert np.array_equal(a[keep], want[keep])


def test_act_refuses_unsupported_shapes():
    from nerve_cl import _nvq
    net, _, obs, _ = _net("unsupported")
    B = 4
    out = (torch.empty(B, 2, dtype=torch.int32, device=_dev()), torch.empty(B, device=_dev()), torch.empty(B, device=_dev()))
    lin = [m for m in net.features if isinstance(m, torch.nn.Linear)]
    with pytest.raises(RuntimeError, match="unsupported network"):
        _nvq.abr_act(obs[:B].to(_dev()), [(m.weight, m.bias) for m in lin], [(m.weight, m.bias) for m in net.policy_heads],
                     (net.value_head.weight, net.value_head.bias), None, 0, True, *out)
    with pytest.raises(RuntimeError, match="fused kernel"):
        net.act(obs[:B].to(_dev()), fused=True)
    # weights the kernel would stride or read wrongly are refused before the launch
    from nerve_cl.abr import ActorCritic
    good = ActorCritic(7, (5, 5), (64, 64)).to(_dev())
    with pytest.raises(AssertionError, match="after a width of 9"):
        good.act(torch.rand(B, 9, device=_dev()))
    with pytest.raises(AssertionError, match="fp32 weights"):
        ActorCritic(7, (5, 5), (64, 64)).to(_dev()).double().act(torch.rand(B, 7, device=_dev()))


def test_act_sampling_many():
    """2 x 1000 samples of the default network against the inverse CDF of the device's own head outputs"""
    _, heads, _ = NETS["default"]
    net, _, obs, _ = _net("default")
    B, seed = 1000, 4
    counters = torch.arange(B, dtype=torch.int64) % 17
    a, lp, v, x = net.act(obs.to(_dev()), counters.to(_dev()), seed=seed, return_head_outputs=True)
    u = np.array([O.uniforms(seed, e, int(counters[e]), 1)[:2] for e in range(B)])
    want, want_lp, margin = O.sample(x.cpu().numpy(), heads, u)
    keep = margin >= 1e-5
    assert (~keep).sum() <= 0.01 * keep.size, f"{(~keep).sum()} samples within 1e-5 of a CDF boundary"
    assert np.array_equal(a.cpu().numpy()[keep], want[keep])
    assert len(np.unique(a.cpu().numpy()[:, 0])) > 1 and len(np.unique(a.cpu().numpy()[:, 1])) > 1
    rows = keep.all(axis=1)
    assert np.abs(lp.cpu().numpy()[rows] - want_lp[rows]).max() <= 1e-5


def test_act_deterministic_and_draws():
    from nerve_cl.abr import ActorCritic
    torch.manual_seed(2)
    net = ActorCritic(7, (5, 5), (64, 64))
    with torch.no_grad():                       # logits 1 and 3 of head 0 are the same function with the largest bias: a tie
        net.policy_heads[0].weight[3] = net.policy_heads[0].weight[1]
        net.policy_heads[0].bias[1] = net.policy_heads[0].bias[3] = 50.0
    net = net.to(_dev())
    obs = torch.rand(70, 7, generator=torch.Generator().manual_seed(3)).to(_dev())
    a, lp, v, x = net.act(obs, deterministic=True, return_head_outputs=True)
    assert bool((x[:, 1] == x[:, 3]).all()), "the tie must be exact"
    assert np.array_equal(a[:, 0].cpu().numpy(), np.ones(70, dtype=np.int32))
    assert torch.equal(a[:, 1].long(), x[:, 5:10].argmax(dim=-1))
    a_null, _, _ = net.act(obs, counters=None)
    assert torch.equal(a_null, a)
    net2, _, obs2, _ = _net("default")
    obs2 = obs2[:70].to(_dev())
    c = torch.arange(70, dtype=torch.int64, device=_dev())
    s1, s2, s3 = net2.act(obs2, c, seed=8), net2.act(obs2, c.clone(), seed=8), net2.act(obs2, c + 1, seed=8)
    assert torch.equal(s1[0], s2[0]) and torch.equal(s1[1], s2[1]) and torch.equal(s1[2], s2[2])
    assert not torch.equal(s1[0], s3[0]) and torch.equal(s1[2], s3[2])


# ---------------------------------------------------------------------------------------------------------------- GAE
def _gae_dev(r, v, d, last, gamma, lam):
    from nerve_cl import _nvq
    t = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float32).contiguous().to(_dev())      # noqa: E731
    ret, adv = torch.empty(r.shape, device=_dev()), torch.empty(r.shape, device=_dev())
    _nvq.abr_gae(t(r), t(v), t(d), t(last), gamma, lam, ret, adv)
    return ret.cpu().numpy().astype(np.float64), adv.cpu().numpy().astype(np.float64)


def _gae_floor(r, v, last):
    """The absolute part of the GAE bound.  delta = r + gamma v' - v cancels, so an element that comes out small still carries the
    rounding of its operands: each of the scan's four fp32 operations per step rounds by at most half an ulp (2^-24 relative) of
    a value no larger than S = max|r| + 2 max|v|, and 1 / (1 - gamma lam) = 17 steps weigh in.  Allowed: 8 x 2^-24 x S, a few
    such roundings, far below a wrong element (of the order of S itself)."""
    S = np.abs(r).max() + 2 * max(np.abs(v).max(), np.abs(last).max())
    return 8 * 2.0 ** -24 * S


def test_gae_matches_oracle():
    rng = np.random.default_rng(0)
    T, N = 5, 3
    r, v = rng.normal(size=(T, N)).astype(np.float32), rng.normal(size=(T, N)).astype(np.float32)
    d = np.zeros((T, N), np.float32)
    d[2, 0] = 1.0          # in the middle of one row
    d[4, 1] = 1.0          # at the last step of another
    last = np.array([0.7, -1.3, 0.4], np.float32)
    ret, adv = _gae_dev(r, v, d, last, 0.99, 0.95)
    o_ret, o_adv = O.gae(r, v, d, last, 0.99, 0.95)
    floor = _gae_floor(r, v, last)
    assert (np.abs(ret - o_ret) <= 1e-6 * np.abs(o_ret) + floor).all()
    assert (np.abs(adv - o_adv) <= 1e-6 * np.abs(o_adv) + floor).all()
    assert adv[4, 1] == np.float32(r[4, 1] - v[4, 1])      # a done at the last step drops the bootstrap value


def test_gae_matches_reference_fixture():
    g = np.load(GOLDEN)
    T = len(g["upd_rewards"])
    ret, adv = _gae_dev(g["upd_rewards"].reshape(T, 1), g["upd_values"].reshape(T, 1), g["upd_dones"].reshape(T, 1).astype(np.float32),
                        np.zeros(1), 0.99, 0.95)
    floor = _gae_floor(g["upd_rewards"], g["upd_values"], np.zeros(1))
    assert (np.abs(ret[:, 0] - g["upd_returns"]) <= 1e-6 * np.abs(g["upd_returns"]) + floor).all()
    assert (np.abs(adv[:, 0] - g["upd_advantages"]) <= 1e-6 * np.abs(g["upd_advantages"]) + floor).all()


# ---------------------------------------------------------------------------------------------------------------- PPO loss
CLIP, VC, EC = 0.2, 0.5, 0.01


def _ppo_inputs(M, heads):
    rng = np.random.default_rng(M + heads[0])
    P = sum(heads) + 1
    x = rng.normal(size=(M, P)).astype(np.float32) * 1.5
    actions = np.stack([rng.integers(0, n, size=M) for n in heads], axis=1).astype(np.int32)
    new = O.log_prob_of(x, heads, actions)
    old = (new - rng.uniform(np.log(0.5), np.log(1.6), size=M)).astype(np.float32)
    adv = rng.normal(size=M).astype(np.float32) * 2 + 0.3
    ret = rng.normal(size=M).astype(np.float32)
    return x, actions, old, adv, ret


@pytest.mark.parametrize("heads", [(5, 5), (3, 7)])
@pytest.mark.parametrize("M", [64, 1000])
def test_ppo_loss_matches_oracle(M, heads):
    from nerve_cl import ops
    x, actions, old, adv, ret = _ppo_inputs(M, heads)
    o_loss, o_x, o_stats, ratio = O.ppo_loss(x, heads, actions, old, adv, ret, CLIP, VC, EC)
    o_loss.backward()
    ratio = ratio.numpy()
    assert ratio.min() < 0.7 and ratio.max() > 1.4 and (adv > 0).any() and (adv < 0).any()
    assert np.abs(ratio - (1 - CLIP)).min() > 1e-4 and np.abs(ratio - (1 + CLIP)).min() > 1e-4, "precondition: a ratio at a clip edge"
    # the same composition in fp32 by torch on the CPU: the error a correct fp32 evaluation makes
    xc = torch.tensor(x, requires_grad=True)
    c_loss, c_stats = ops.ppo_loss_composition(xc, heads, torch.tensor(actions), torch.tensor(old), torch.tensor(adv),
                                               torch.tensor(ret), CLIP, VC, EC, dtype=torch.float32)
    c_loss.backward()
    dev = lambda a: torch.tensor(a).to(_dev())      # noqa: E731
    xd = dev(x).requires_grad_(True)
    args = (dev(actions), dev(old), dev(adv), dev(ret), CLIP, VC, EC)
    loss, stats = ops.ppo_loss(xd, *args, heads=heads, return_stats=True)
    loss.backward()
    stats_h = stats.cpu().numpy()
    for i, k in enumerate(ops.PPO_STATS):
        tol = 8.0 * abs(float(c_stats[i]) - o_stats[k])
        print(f"ppo_loss M={M} heads={heads} {k}: err {abs(stats_h[i] - o_stats[k]):.3e}, torch CPU fp32 err {tol / 8:.3e}")
        assert abs(stats_h[i] - o_stats[k]) <= tol, k
    assert loss.item() == stats_h[0]
    g_ref = o_x.grad.numpy()
    tol = 8.0 * np.abs(xc.grad.numpy() - g_ref).max()
    err = np.abs(xd.grad.cpu().numpy() - g_ref).max()
    print(f"    gradient err {err:.3e}, torch CPU fp32 err {tol / 8:.3e}")
    assert err <= tol
    # as the forward's tuple, bit-identical run to run, and grad_output scales the stored gradient
    off, parts = 0, []
    for n in list(heads) + [1]:
        parts.append(dev(x[:, off:off + n]).requires_grad_(True))
        off += n
    loss2, stats2 = ops.ppo_loss(tuple(parts), *args, return_stats=True)
    (3.0 * loss2).backward()
    assert torch.equal(stats2, stats)
    assert torch.equal(torch.cat([p.grad for p in parts], dim=-1), xd.grad * 3.0)


# ---------------------------------------------------------------------------------------------------------------- agent
def _agent(n_envs=8, max_steps=6, seed=5):
    from nerve_cl.abr import ABRConfig, PPOAgent, VecStreamingEnv
    torch.manual_seed(1)
    agent = PPOAgent(7, (5, 5), ABRConfig(hidden_dims=(64, 64)), device=_dev())
    env = VecStreamingEnv(n_envs, max_steps=max_steps, seed=seed, device=_dev())
    return agent, env


def test_agent_collect_and_update():
    agent, env = _agent()
    assert agent.fused
    T, N = 16, 8
    ro = agent.collect(env, T)
    torch.cuda.synchronize()
    actions = ro["actions"].cpu().numpy()
    ref = O.vec_rollout(N, actions, env.seed, 6)
    done = (ref["terminated"] | ref["truncated"]).astype(np.float32)
    assert done.any()
    assert np.array_equal(ro["rewards"].cpu().numpy(), ref["reward"].astype(np.float32))
    assert np.array_equal(ro["dones"].cpu().numpy(), done)
    assert _ulps(ro["obs"][1:].cpu().numpy(), ref["obs"]).max() <= 1
    # the stored actions are the inverse CDF of the network's outputs on the stored observations with the draw of counter t + 1
    left_out = 0
    for t in range(T):
        _, lp, v, x = agent.network.act(ro["obs"][t], deterministic=True, return_head_outputs=True)
        assert torch.equal(v, ro["values"][t])
        u = np.array([O.uniforms(env.seed, e, t + 1, 1)[:2] for e in range(N)])
        want, want_lp, margin = O.sample(x.cpu().numpy(), (5, 5), u)
        keep = margin >= 1e-5
        left_out += (~keep).sum()
        assert np.array_equal(actions[t][keep], want[keep]), t
        assert np.abs(ro["log_probs"][t].cpu().numpy() - O.log_prob_of(x.cpu().numpy(), (5, 5), actions[t])).max() <= 1e-5
    assert left_out <= 2
    before = [p.detach().clone() for p in agent.network.parameters()]
    values, last = ro["values"].cpu().numpy(), ro["last_values"].cpu().numpy()
    metrics = agent.update()
    o_ret, o_adv = O.gae(ref["reward"].astype(np.float32), values, done, last, 0.99, 0.95)
    floor = _gae_floor(ref["reward"], values, last)
    assert (np.abs(ro["returns"].cpu().numpy() - o_ret) <= 1e-6 * np.abs(o_ret) + floor).all()
    assert (np.abs(ro["advantages"].cpu().numpy() - o_adv) <= 1e-6 * np.abs(o_adv) + floor).all()
    for k in ("loss", "policy_loss", "value_loss", "entropy", "approx_kl", "clip_fraction"):
        assert np.isfinite(metrics[k]), (k, metrics)
    assert all(not torch.equal(b, p) for b, p in zip(before, agent.network.parameters()))


def test_unsupported_width_says_so_and_still_collects():
    from nerve_cl.abr import ABRConfig, PPOAgent, VecStreamingEnv
    with pytest.warns(UserWarning, match="torch composition"):
        agent = PPOAgent(7, (5, 5), ABRConfig(hidden_dims=(48, 48), ppo_epochs=1), device=_dev())
    assert not agent.fused
    env = VecStreamingEnv(8, max_steps=6, seed=5, device=_dev())
    ro = agent.collect(env, 8)
    ref = O.vec_rollout(8, ro["actions"].cpu().numpy(), 5, 6)
    assert np.array_equal(ro["rewards"].cpu().numpy(), ref["reward"].astype(np.float32))
    assert np.isfinite(agent.update()["loss"])


def test_collect_reads_nothing_back():
    agent, env = _agent()
    agent.collect(env, 4)                           # allocates the rollout
    acts = torch.zeros(8, 2, dtype=torch.int32, device=_dev())
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        agent.collect(env, 4)
        env.step(acts)
        agent.network.act(env.obs, env.counters, seed=3)
        with pytest.raises(RuntimeError):
            env.obs.sum().item()                    # the control: a read-back does raise
    finally:
        torch.cuda.set_sync_debug_mode("default")


def test_collect_graph_replay_is_bit_equal():
    agent, env = _agent()
    T = 16
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        agent.collect(env, T)                       # allocates the rollout outside the capture
    torch.cuda.current_stream().wait_stream(side)
    saved = [t.clone() for t in (env.state, env.counters, env.obs, env.finished)]

    def restore():
        for dst, src in zip((env.state, env.counters, env.obs, env.finished), saved):
            dst.copy_(src)

    keys = ("obs", "actions", "log_probs", "values", "rewards", "dones", "last_values")
    eager = {k: v.clone() for k, v in agent.collect(env, T).items() if k in keys}
    end_state = env.state.clone()
    restore()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ro = agent.collect(env, T)
    restore()
    for k in keys:                                  # (row T of obs is the environment's restored observation)
        (ro[k][:T] if k == "obs" else ro[k]).zero_()
    graph.replay()
    torch.cuda.synchronize()
    for k in keys:
        assert torch.equal(ro[k], eager[k]), k
    assert torch.equal(env.state, end_state)


def test_single_stream_agent_on_the_device():
    """the host-side loop (one StreamingEnv, one decision per call) with the network on the GPU: act on a batch of one, the
    fused loss in update()"""
    from nerve_cl.abr import ABRConfig, PPOAgent, StreamingEnv
    torch.manual_seed(3)
    agent = PPOAgent(7, (5, 5), ABRConfig(ppo_epochs=2), device="cuda", seed=6)
    env = StreamingEnv(max_steps=10)
    obs, _ = env.reset(seed=1)
    for i in range(40):
        action = agent.select_action(obs)
        assert action.shape == (2,) and 0 <= action.min() and action.max() < 5
        u = O.uniforms(6, 0, i, 1)[:2]
        with torch.no_grad():
            x = torch.cat(agent.network(torch.as_tensor(obs).reshape(1, -1).cuda()), dim=-1).cpu().numpy()
        want, _, margin = O.sample(x, (5, 5), np.array([u]))
        assert (margin < 1e-5).any() or np.array_equal(want[0], action), i
        obs, reward, term, trunc, _ = env.step(action)
        agent.store_transition(action, reward, term or trunc)
        if term or trunc:
            obs, _ = env.reset()
    before = [p.detach().clone() for p in agent.network.parameters()]
    metrics = agent.update()
    assert np.isfinite(metrics["loss"]) and np.isfinite(metrics["approx_kl"])
    assert all(not torch.equal(b, p) for b, p in zip(before, agent.network.parameters()))
