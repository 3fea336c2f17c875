"""Write tests/golden/abr_reference.npz and tests/golden/abr_reference_checkpoint.pt from the reference's nerve_cl/abr.

    python tools/make_abr_goldens.py /path/to/reference

Runs where the reference checkout is; the outputs hold data only (arrays and a torch checkpoint).  The reference's two files are
loaded by path.  `gymnasium` is not needed: a few-line stand-in is registered in sys.modules for the import, and
np.random.uniform is wrapped so that every draw is recorded in order (the environment draws from numpy's global state).

Contents of the npz
  ep{0,1,2}_*   three episodes: draws (every np.random.uniform value in call order: reset bandwidth, reset complexity, then per
                step bandwidth factor, complexity), actions, obs (the reset observation first), rewards, terminated, truncated and
                the info values vmaf / rebuffer / bandwidth / buffer; max_steps in ep*_max_steps.
                ep0: random actions, max_steps 20.  ep1: enhancement 4 at every step, ends by battery truncation.
                ep2: the top bitrate at every step (rebuffering), max_steps 15.
  net_*         ActorCritic(7, (5, 5), (256, 256)) state dict (net_keys, net_p{i}), 16 observations and its outputs on them.
  upd_*         one update() of PPOAgent(7, (5, 5), hidden (64, 64)) on a 64-transition buffer it collected itself: the state dict
                before and after the ten epochs, the buffer, the GAE returns / advantages, every epoch's loss, the returned
                mean loss; upd_spread = max |difference| of the final parameters between runs with 1 and 4 torch threads.
"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(REPO, "tests", "golden", "abr_reference.npz")
OUT_CKPT = os.path.join(REPO, "tests", "golden", "abr_reference_checkpoint.pt")


def _gym_stand_in():
    gym = types.ModuleType("gymnasium")
    spaces = types.ModuleType("gymnasium.spaces")

    class Env:
        def reset(self, seed=None, options=None):
            return None

    class MultiDiscrete:
        def __init__(self, nvec):
            self.nvec = np.asarray(nvec, dtype=np.int64)
            self.shape = self.nvec.shape
            self.dtype = np.int64

        def sample(self):
            return np.array([np.random.randint(n) for n in self.nvec], dtype=np.int64)

    class Box:
        def __init__(self, low, high, shape, dtype):
            self.low, self.high, self.shape, self.dtype = low, high, shape, dtype

    gym.Env, gym.spaces = Env, spaces
    spaces.MultiDiscrete, spaces.Box = MultiDiscrete, Box
    sys.modules["gymnasium"], sys.modules["gymnasium.spaces"] = gym, spaces


def _load(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


class Recorder:
    def __init__(self):
        self.draws = []
        self._orig = np.random.uniform

    def __call__(self, *a, **k):
        v = self._orig(*a, **k)
        self.draws.append(float(v))
        return v


def episode(envmod, rec, seed, max_steps, policy):
    env = envmod.StreamingEnv(max_steps=max_steps)
    np.random.seed(seed)
    rec.draws.clear()
    obs, _ = env.reset()
    out = dict(obs=[obs], actions=[], rewards=[], terminated=[], truncated=[], vmaf=[], rebuffer=[], bandwidth=[], buffer=[])
    rng = np.random.RandomState(1000 + seed)
    while True:
        a = policy(rng)
        obs, r, term, trunc, info = env.step(a)
        out["obs"].append(obs)
        out["actions"].append(a)
        out["rewards"].append(float(r))
        out["terminated"].append(bool(term))
        out["truncated"].append(bool(trunc))
        for k in ("vmaf", "rebuffer", "bandwidth", "buffer"):
            out[k].append(float(info[k]))
        if term or trunc:
            break
    res = {k: np.asarray(v) for k, v in out.items()}
    res["obs"] = res["obs"].astype(np.float32)
    res["actions"] = res["actions"].astype(np.int64)
    for k in ("rewards", "vmaf", "rebuffer", "bandwidth", "buffer"):
        res[k] = res[k].astype(np.float64)
    res["draws"] = np.asarray(rec.draws, dtype=np.float64)
    res["max_steps"] = np.int64(max_steps)
    return res


def run_update(agentmod, envmod, threads):
    """collect 64 transitions with the reference loop, then one update(); returns everything the fixture records"""
    torch.set_num_threads(threads)
    torch.manual_seed(7)
    np.random.seed(11)
    cfg = agentmod.ABRConfig(hidden_dims=(64, 64))
    agent = agentmod.PPOAgent(7, (5, 5), cfg)
    before = {k: v.clone() for k, v in agent.network.state_dict().items()}
    env = envmod.StreamingEnv(max_steps=25)
    obs, _ = env.reset()
    for _ in range(64):
        a = agent.select_action(obs)
        obs, r, term, trunc, _ = env.step(a)
        agent.store_transition(a, r, term or trunc)
        if term or trunc:
            obs, _ = env.reset()
    buf = {k: list(v) for k, v in agent.buffer.items()}
    returns, advantages = agent._compute_gae()
    losses = []
    orig_backward = torch.Tensor.backward

    def recording_backward(self, *a, **k):
        losses.append(float(self.item()))
        return orig_backward(self, *a, **k)

    torch.Tensor.backward = recording_backward
    try:
        res = agent.update()
    finally:
        torch.Tensor.backward = orig_backward
    after = {k: v.clone() for k, v in agent.network.state_dict().items()}
    return dict(agent=agent, before=before, after=after, buf=buf, returns=np.asarray(returns, dtype=np.float64),
                advantages=np.asarray(advantages, dtype=np.float64), losses=np.asarray(losses, dtype=np.float64),
                mean_loss=float(res["loss"]))


def main():
    ref = sys.argv[1] if len(sys.argv) > 1 else os.environ.get("NERVE_CL_REFERENCE", "")
    if not os.path.isdir(os.path.join(ref, "nerve_cl", "abr")):
        raise SystemExit("usage: make_abr_goldens.py /path/to/reference")
    _gym_stand_in()
    rec = Recorder()
    np.random.uniform = rec
    envmod = _load(os.path.join(ref, "nerve_cl", "abr", "environment.py"), "_ref_abr_environment")
    agentmod = _load(os.path.join(ref, "nerve_cl", "abr", "agent.py"), "_ref_abr_agent")
    data = {}

    eps = [episode(envmod, rec, 3, 20, lambda rng: np.array([rng.randint(5), rng.randint(5)])),
           episode(envmod, rec, 4, 100, lambda rng: np.array([rng.randint(5), 4])),
           episode(envmod, rec, 5, 15, lambda rng: np.array([4, rng.randint(5)]))]
    assert eps[0]["terminated"][-1] and not eps[0]["truncated"][-1]
    assert eps[1]["truncated"][-1] and not eps[1]["terminated"][-1]
    assert eps[2]["rebuffer"].max() > 0.0
    for i, ep in enumerate(eps):
        for k, v in ep.items():
            data[f"ep{i}_{k}"] = v

    torch.manual_seed(0)
    net = agentmod.ActorCritic(7, (5, 5), (256, 256))
    sd = net.state_dict()
    data["net_keys"] = np.array(list(sd.keys()))
    for i, v in enumerate(sd.values()):
        data[f"net_p{i}"] = v.numpy()
    g = torch.Generator().manual_seed(1)
    obs = torch.rand(16, 7, generator=g)
    with torch.no_grad():
        outs = net(obs)
    data["net_obs"] = obs.numpy()
    for i, o in enumerate(outs):
        data[f"net_out{i}"] = o.numpy()

    u1 = run_update(agentmod, envmod, 1)
    u4 = run_update(agentmod, envmod, 4)
    spread = max(float((u1["after"][k] - u4["after"][k]).abs().max()) for k in u1["after"])
    data["upd_keys"] = np.array(list(u1["before"].keys()))
    for i, k in enumerate(u1["before"]):
        data[f"upd_before{i}"] = u1["before"][k].numpy()
        data[f"upd_after{i}"] = u1["after"][k].numpy()
    b = u1["buf"]
    data["upd_obs"] = np.asarray(b["obs"], dtype=np.float32)
    data["upd_actions"] = np.asarray(b["actions"], dtype=np.int64)
    data["upd_rewards"] = np.asarray(b["rewards"], dtype=np.float64)
    data["upd_values"] = np.asarray(b["values"], dtype=np.float64)
    data["upd_log_probs"] = np.asarray(b["log_probs"], dtype=np.float64)
    data["upd_dones"] = np.asarray(b["dones"], dtype=np.bool_)
    data["upd_returns"], data["upd_advantages"] = u1["returns"], u1["advantages"]
    data["upd_losses"], data["upd_mean_loss"] = u1["losses"], np.float64(u1["mean_loss"])
    data["upd_spread"] = np.float64(spread)
    data["upd_loss_spread"] = np.float64(np.abs(u1["losses"] - u4["losses"]).max())
    assert data["upd_dones"].any()

    np.savez_compressed(OUT, **data)
    u1["agent"].save(OUT_CKPT)
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes), {OUT_CKPT} ({os.path.getsize(OUT_CKPT)} bytes); "
          f"thread spread of the updated parameters {spread:.3e}, of the losses {float(data['upd_loss_spread']):.3e}")


if __name__ == "__main__":
    main()
