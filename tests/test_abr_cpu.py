"""CPU: the ABR package against the reference's recorded behaviour (tests/golden/abr_reference.npz, written by
tools/make_abr_goldens.py from the reference's own environment.py and agent.py) and against tests/_abr_oracle.py.

The fixture holds three reference episodes with every np.random.uniform draw in call order (one ends by step count, one by
battery truncation, one rebuffers), an ActorCritic(7, (5, 5), (256, 256)) with its outputs, one update() of a 64-transition
buffer on hidden (64, 64) and the checkpoint its save() wrote."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import _abr_oracle as O  # noqa: E402

GOLDEN = os.path.join(HERE, "golden", "abr_reference.npz")
CKPT = os.path.join(HERE, "golden", "abr_reference_checkpoint.pt")


def _g():
    return np.load(GOLDEN)


def test_oracle_reproduces_reference_episodes():
    g = _g()
    kinds = []
    for i in range(3):
        draws, actions, max_steps = g[f"ep{i}_draws"], g[f"ep{i}_actions"], int(g[f"ep{i}_max_steps"])
        s, obs = O.reset(draws[0], draws[1], max_steps=max_steps)
        assert np.array_equal(obs.view(np.int32), g[f"ep{i}_obs"][0].view(np.int32))
        for t in range(len(actions)):
            s, obs, r, term, trunc, info = O.step(s, actions[t], draws[2 + 2 * t], draws[3 + 2 * t], max_steps=max_steps)
            assert obs.dtype == np.float32 and np.array_equal(obs.view(np.int32), g[f"ep{i}_obs"][t + 1].view(np.int32)), (i, t)
            assert r == g[f"ep{i}_rewards"][t], (i, t)
            assert term == g[f"ep{i}_terminated"][t] and trunc == g[f"ep{i}_truncated"][t], (i, t)
            for k in ("vmaf", "rebuffer", "bandwidth", "buffer"):
                assert info[k] == g[f"ep{i}_{k}"][t], (i, t, k)
        assert len(draws) == 2 + 2 * len(actions)
        kinds.append((bool(term), bool(trunc)))
    assert (True, False) in kinds and (False, True) in kinds and g["ep2_rebuffer"].max() > 0


class _Replay:
    """a Generator stand-in that replays recorded draws, to drive StreamingEnv with the reference's numbers"""

    def __init__(self, draws):
        self.draws, self.i = list(draws), 0

    def uniform(self, low, high):
        v = self.draws[self.i]
        assert low <= v <= high
        self.i += 1
        return v


def test_streaming_env_reproduces_reference_episodes():
    from nerve_cl.abr import StreamingEnv
    g = _g()
    for i in range(3):
        env = StreamingEnv(max_steps=int(g[f"ep{i}_max_steps"]))
        env.np_random = _Replay(g[f"ep{i}_draws"])
        obs, info = env.reset()
        assert info == {} and np.array_equal(obs, g[f"ep{i}_obs"][0])
        for t, a in enumerate(g[f"ep{i}_actions"]):
            obs, r, term, trunc, info = env.step(a)
            assert np.array_equal(obs, g[f"ep{i}_obs"][t + 1]) and r == g[f"ep{i}_rewards"][t]
            assert term == g[f"ep{i}_terminated"][t] and trunc == g[f"ep{i}_truncated"][t]
            assert set(info) == {"vmaf", "rebuffer", "bandwidth", "buffer"}
            assert all(info[k] == g[f"ep{i}_{k}"][t] for k in info)


def test_streaming_env_surface():
    """the shapes, types and keys a user of the reference's environment relies on, and an episode's length under random actions"""
    from nerve_cl.abr import StreamingEnv
    env = StreamingEnv()
    first, extra = env.reset()
    assert extra == {} and first.shape == (7,) and first.dtype == np.float32
    out = env.step(np.array([2, 2]))
    assert len(out) == 5
    obs, reward, terminated, truncated, info = out
    assert obs.shape == (7,) and obs.dtype == np.float32 and type(reward) is float
    assert type(terminated) is bool and type(truncated) is bool and not terminated and not truncated
    assert sorted(info) == ["bandwidth", "buffer", "rebuffer", "vmaf"] and info["vmaf"] == 50 + (2 / 5) * 40 + 0.5 * 10
    # 20 steps cost at most 20 * 0.03 of battery, so only the step count can end this episode
    short = StreamingEnv(max_steps=20)
    short.reset()
    lengths = 0
    while True:
        _, _, terminated, truncated, _ = short.step(short.action_space.sample())
        lengths += 1
        if terminated or truncated:
            break
    assert lengths == 20 and terminated and not truncated


def test_spaces_and_seeding():
    from nerve_cl.abr import StreamingEnv
    env = StreamingEnv()
    assert env.action_space.shape == (2,) and list(env.action_space.nvec) == [5, 5] and env.action_space.dtype == np.int64
    assert env.observation_space.shape == (7,) and env.observation_space.dtype == np.float32
    samples = np.array([env.action_space.sample() for _ in range(200)])
    assert samples.shape == (200, 2) and samples.min() == 0 and samples.max() == 4
    a, _ = env.reset(seed=3)
    b, _ = StreamingEnv().reset(seed=3)
    assert np.array_equal(a, b) and a.min() >= 0.0 and a.max() <= 1.0
    import nerve_cl
    assert nerve_cl.StreamingEnv is StreamingEnv and "gymnasium" not in sys.modules


def _fixture_net(g):
    from nerve_cl.abr import ActorCritic
    net = ActorCritic(7, (5, 5), (256, 256))
    sd = {str(k): torch.from_numpy(g[f"net_p{i}"]) for i, k in enumerate(g["net_keys"])}
    assert list(net.state_dict().keys()) == list(sd.keys())
    net.load_state_dict(sd)
    return net, sd


def test_actor_critic_reproduces_reference_outputs():
    g = _g()
    net, sd = _fixture_net(g)
    with torch.no_grad():
        outs = net(torch.from_numpy(g["net_obs"]))
    assert len(outs) == 3 and tuple(outs[2].shape) == (16, 1)
    ref = O.mlp({k: v.numpy() for k, v in sd.items()}, g["net_obs"], 2, 2)
    off = 0
    for i, o in enumerate(outs):
        want = g[f"net_out{i}"]
        # fp32 rounding: the same GEMMs may be blocked differently; both sit within a few ulps of the float64 value
        assert np.abs(o.numpy() - want).max() <= 8 * np.finfo(np.float32).eps * max(1.0, np.abs(want).max())
        assert np.abs(want - ref[:, off:off + want.shape[1]]).max() <= 1e-5
        off += want.shape[1]


def _fixture_agent(g):
    from nerve_cl.abr import ABRConfig, PPOAgent
    agent = PPOAgent(7, (5, 5), ABRConfig(hidden_dims=(64, 64)), device="cpu")
    agent.network.load_state_dict({str(k): torch.from_numpy(g[f"upd_before{i}"]) for i, k in enumerate(g["upd_keys"])})
    agent.buffer = dict(obs=list(g["upd_obs"]), actions=list(g["upd_actions"]), rewards=[float(x) for x in g["upd_rewards"]],
                        values=[float(x) for x in g["upd_values"]], log_probs=[float(x) for x in g["upd_log_probs"]],
                        dones=[bool(x) for x in g["upd_dones"]])
    return agent


def test_agent_update_reproduces_reference():
    """GAE exactly in float64; every epoch's loss and the ten-epoch parameters within 8 x the spread the reference itself shows
    between runs with 1 and 4 torch threads on this fixture.  That spread was measured as 0.0 for the parameters and 0.0 for the
    losses (upd_spread / upd_loss_spread in the fixture: a 64 x 64 network is below torch's threading threshold), so the bound
    is equality.  Equality ties this test to the CPU GEMM path of the host that wrote the fixture (it has held on the x86-64
    hosts tried): on a host with another ISA or BLAS, regenerate the fixture there with tools/make_abr_goldens.py."""
    g = _g()
    assert float(g["upd_spread"]) == 0.0 and float(g["upd_loss_spread"]) == 0.0
    agent = _fixture_agent(g)
    from nerve_cl.abr.agent import gae_stream
    returns, advantages = gae_stream(agent.buffer["rewards"], agent.buffer["values"], agent.buffer["dones"], 0.99, 0.95)
    assert np.array_equal(returns, g["upd_returns"]) and np.array_equal(advantages, g["upd_advantages"])
    o_ret, o_adv = O.gae(g["upd_rewards"][:, None], g["upd_values"][:, None], g["upd_dones"][:, None], np.zeros(1), 0.99, 0.95)
    assert np.allclose(o_ret[:, 0], g["upd_returns"], rtol=1e-13) and np.allclose(o_adv[:, 0], g["upd_advantages"], rtol=1e-12, atol=1e-13)
    first = _fixture_agent(g)
    first.config.ppo_epochs = 1
    assert abs(first.update()["loss"] - g["upd_losses"][0]) <= 8 * float(g["upd_loss_spread"])
    metrics = agent.update()
    assert abs(metrics["loss"] - float(g["upd_mean_loss"])) <= 8 * float(g["upd_loss_spread"])
    assert all(len(v) == 0 for v in agent.buffer.values())
    for i, (k, v) in enumerate(agent.network.state_dict().items()):
        assert (v - torch.from_numpy(g[f"upd_after{i}"])).abs().max().item() <= 8 * float(g["upd_spread"]), k
    for k in ("policy_loss", "value_loss", "entropy", "approx_kl", "clip_fraction"):
        assert np.isfinite(metrics[k])


def test_reference_checkpoint_loads_and_key_sets_match(tmp_path):
    from nerve_cl.abr import ABRConfig, PPOAgent
    g = _g()
    agent = PPOAgent(7, (5, 5), ABRConfig(hidden_dims=(64, 64)))
    agent.load(CKPT)
    for i, (k, v) in enumerate(agent.network.state_dict().items()):
        assert torch.equal(v, torch.from_numpy(g[f"upd_after{i}"])), k
    path = str(tmp_path / "agent.pt")
    agent.save(path)
    ours, theirs = torch.load(path), torch.load(CKPT)
    assert set(ours) == set(theirs) == {"network", "optimizer"}
    assert list(ours["network"].keys()) == list(theirs["network"].keys())
    assert set(ours["optimizer"]) == set(theirs["optimizer"])
    assert ours["optimizer"]["param_groups"][0].keys() == theirs["optimizer"]["param_groups"][0].keys()
    assert set(ours["optimizer"]["state"]) == set(theirs["optimizer"]["state"])
    agent2 = PPOAgent(7, (5, 5), ABRConfig(hidden_dims=(64, 64)))
    agent2.load(path)


def test_single_stream_agent_on_the_host():
    """select_action / store_transition / update over one StreamingEnv: valid actions, a buffer that fills and empties, draws that
    follow the agent's seed, deterministic = argmax"""
    from nerve_cl.abr import ABRConfig, PPOAgent, StreamingEnv
    cfg = ABRConfig()
    assert (cfg.hidden_dims, cfg.learning_rate, cfg.gamma, cfg.gae_lambda, cfg.clip_ratio, cfg.value_coef, cfg.entropy_coef,
            cfg.ppo_epochs, cfg.max_grad_norm) == ((256, 256), 3e-4, 0.99, 0.95, 0.2, 0.5, 0.01, 10, 0.5)
    torch.manual_seed(4)
    small = ABRConfig(hidden_dims=(32, 32), ppo_epochs=3)
    agent, twin = PPOAgent(7, (5, 5), small, seed=9), PPOAgent(7, (5, 5), small, seed=9)
    twin.network.load_state_dict(agent.network.state_dict())
    env = StreamingEnv(max_steps=10)
    obs, _ = env.reset(seed=2)
    picks = []
    for i in range(48):
        action = agent.select_action(obs)
        assert np.array_equal(action, twin.select_action(obs))
        assert action.shape == (2,) and 0 <= action[0] < 5 and 0 <= action[1] < 5
        picks.append(tuple(action))
        obs, reward, term, trunc, _ = env.step(action)
        agent.store_transition(action, reward, term or trunc)
        if term or trunc:
            obs, _ = env.reset()
    assert len(set(picks)) > 5 and all(len(v) == 48 for v in agent.buffer.values())
    greedy = agent.select_action(obs, deterministic=True)
    with torch.no_grad():
        outs = agent.network(torch.as_tensor(obs).reshape(1, -1))
    assert [int(o.argmax()) for o in outs[:2]] == list(greedy) and len(agent.buffer["obs"]) == 48
    before = [p.detach().clone() for p in agent.network.parameters()]
    metrics = agent.update()
    assert np.isfinite(metrics["loss"]) and all(len(v) == 0 for v in agent.buffer.values())
    assert all(not torch.equal(b, p) for b, p in zip(before, agent.network.parameters()))


def test_vec_env_cpu_matches_oracle():
    from nerve_cl.abr import VecStreamingEnv
    N, T, seed, max_steps = 7, 45, 3, 36
    rng = np.random.default_rng(0)
    actions = rng.integers(0, 5, size=(T, N, 2))
    actions[:, 0, 1] = 4
    ref = O.vec_rollout(N, actions, seed, max_steps)
    assert ref["terminated"].any() and ref["truncated"].any()
    env = VecStreamingEnv(N, max_steps=max_steps, seed=seed, device="cpu")
    assert np.array_equal(env.obs.numpy(), ref["obs0"])
    for t in range(T):
        obs, reward, term, trunc, info = env.step(torch.as_tensor(actions[t], dtype=torch.int32))
        assert obs.dtype == torch.float32 and reward.dtype == torch.float64 and term.dtype == torch.bool
        assert np.array_equal(obs.numpy(), ref["obs"][t]) and np.array_equal(reward.numpy(), ref["reward"][t]), t
        assert np.array_equal(term.numpy(), ref["terminated"][t]) and np.array_equal(trunc.numpy(), ref["truncated"][t]), t
        for k in ("vmaf", "rebuffer", "bandwidth", "buffer", "episode_return"):
            assert np.array_equal(info[k].numpy(), ref[k][t]), (t, k)
    assert (env.counters.numpy() == T + 1).all()
    again = env.reset(seed=seed)
    assert np.array_equal(again.numpy(), ref["obs0"])


def test_act_cpu_matches_oracle():
    from nerve_cl.abr import ActorCritic
    from nerve_cl.abr.agent import philox_uniforms
    torch.manual_seed(0)
    net = ActorCritic(7, (3, 7), (64, 32))
    assert not net.act.__doc__ is None
    B, seed = 40, 12
    obs = torch.rand(B, 7)
    counters = torch.arange(B, dtype=torch.int64) + (1 << 33)          # the high counter word is in play
    u_t = philox_uniforms(torch.arange(B), counters, 1, seed).numpy()
    u = np.array([O.uniforms(seed, e, int(counters[e]), 1) for e in range(B)])
    assert np.array_equal(u_t, u)
    a, lp, v, x = net.act(obs, counters, seed=seed, return_head_outputs=True)
    want, want_lp, margin = O.sample(x.numpy(), (3, 7), u[:, :2])
    keep = margin >= 1e-5
    assert keep.mean() >= 0.99 and np.array_equal(a.numpy()[keep], want[keep])
    assert np.abs(lp.numpy() - O.log_prob_of(x.numpy(), (3, 7), a.numpy())).max() <= 1e-5
    a_det, _, _ = net.act(obs, deterministic=True)
    assert torch.equal(a_det[:, 0].long(), x[:, :3].argmax(-1)) and torch.equal(a_det[:, 1].long(), x[:, 3:10].argmax(-1))


def test_ppo_loss_cpu_matches_oracle():
    from nerve_cl import ops
    rng = np.random.default_rng(1)
    for M, heads in ((64, (5, 5)), (257, (3, 7))):
        P = sum(heads) + 1
        x = rng.normal(size=(M, P)).astype(np.float32)
        actions = np.stack([rng.integers(0, n, size=M) for n in heads], axis=1).astype(np.int32)
        old = (O.log_prob_of(x, heads, actions) - rng.uniform(np.log(0.5), np.log(1.6), size=M)).astype(np.float32)
        adv, ret = rng.normal(size=M).astype(np.float32), rng.normal(size=M).astype(np.float32)
        o_loss, o_x, o_stats, _ = O.ppo_loss(x, heads, actions, old, adv, ret, 0.2, 0.5, 0.01)
        o_loss.backward()
        xt = torch.tensor(x, requires_grad=True)
        loss, stats = ops.ppo_loss(xt, torch.tensor(actions), torch.tensor(old), torch.tensor(adv), torch.tensor(ret), 0.2, 0.5, 0.01,
                                   heads=heads, return_stats=True)
        (2.0 * loss).backward()
        assert loss.dtype == torch.float64 and abs(loss.item() - o_loss.item()) <= 1e-14 * max(1.0, abs(o_loss.item()))
        for i, k in enumerate(ops.PPO_STATS):
            assert abs(stats[i].item() - o_stats[k]) <= 1e-14 * max(1.0, abs(o_stats[k])), k
        # the gradient reaches the fp32 leaf rounded once
        assert np.abs(xt.grad.numpy() - 2.0 * o_x.grad.numpy()).max() <= 2.0 ** -23 * np.abs(o_x.grad.numpy()).max()


def test_collect_and_update_on_cpu():
    from nerve_cl.abr import ABRConfig, PPOAgent, VecStreamingEnv
    torch.manual_seed(0)
    agent = PPOAgent(7, (5, 5), ABRConfig(hidden_dims=(32, 32), ppo_epochs=2), device="cpu")
    assert not agent.fused
    env = VecStreamingEnv(4, max_steps=5, seed=1, device="cpu")
    ro = agent.collect(env, 12)
    ref = O.vec_rollout(4, ro["actions"].numpy(), 1, 5)
    assert np.array_equal(ro["rewards"].numpy(), ref["reward"].astype(np.float32))
    assert np.array_equal(ro["dones"].numpy(), (ref["terminated"] | ref["truncated"]).astype(np.float32))
    before = [p.detach().clone() for p in agent.network.parameters()]
    values, last = ro["values"].numpy().copy(), ro["last_values"].numpy().copy()
    metrics = agent.update()
    o_ret, o_adv = O.gae(ro["rewards"].numpy(), values, ro["dones"].numpy(), last, 0.99, 0.95)
    # elementwise 1e-6 relative plus the absolute floor of the fp32 scan's cancellation (tests/test_abr_gpu.py, _gae_floor)
    floor = 8 * 2.0 ** -24 * (np.abs(ro["rewards"].numpy()).max() + 2 * max(np.abs(values).max(), np.abs(last).max()))
    assert (np.abs(ro["returns"].numpy() - o_ret) <= 1e-6 * np.abs(o_ret) + floor).all()
    assert (np.abs(ro["advantages"].numpy() - o_adv) <= 1e-6 * np.abs(o_adv) + floor).all()
    assert all(np.isfinite(v) for v in metrics.values()) and {"loss", "policy_loss", "clip_fraction"} <= set(metrics)
    assert all(not torch.equal(b, p) for b, p in zip(before, agent.network.parameters()))
