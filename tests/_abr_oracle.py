"""The yardstick of the ABR tests: the streaming environment, the draw assignment, the actor-critic, inverse-CDF sampling, GAE
and the PPO loss in float64, written from the rule alone and independent of nerve_cl (nothing of the package is imported).

Environment.  state = dict(buffer, bandwidth, battery, last_quality, last_vmaf, step_count, total_rebuffer); `reset(bw0, cx)`
and `step(state, action, factor, cx)` take the draws already scaled: bw0 in [2, 15], factor in [0.8, 1.2], cx in [0.3, 0.8].

Draws of the vectorised environment.  Philox4x32-10, key = (seed low, seed high), counter = (e low, e high, t low,
(t high & 0xFFFFFF) | stream << 24) for environment e and its draw counter t; u_j = ((r_j >> 8) + 0.5) 2^-24.  Stream 0 (the
environment): factor = 0.8 + 0.4 u_0, cx = 0.3 + 0.5 u_1 and, when the step ends the episode (or in reset()), the new bandwidth
2 + 13 u_2 and the reset observation's cx = 0.3 + 0.5 u_3.  Stream 1 (the policy): head j samples with u_j.  t advances by one
per step and per reset() call."""
import numpy as np
import torch

BITRATES = (365, 750, 1500, 3000, 6000)
ENH_LEVELS = 5

_M0, _M1, _W0, _W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
_MASK = 0xFFFFFFFF


def philox(c, k):
    """Philox4x32-10 on Python ints: counter (4 words), key (2 words) -> 4 words"""
    c0, c1, c2, c3 = (int(x) & _MASK for x in c)
    k0, k1 = (int(x) & _MASK for x in k)
    for _ in range(10):
        p0, p1 = _M0 * c0, _M1 * c2
        c0, c1, c2, c3 = ((p1 >> 32) ^ c1 ^ k0) & _MASK, p1 & _MASK, ((p0 >> 32) ^ c3 ^ k1) & _MASK, p0 & _MASK
        k0, k1 = (k0 + _W0) & _MASK, (k1 + _W1) & _MASK
    return c0, c1, c2, c3


def uniforms(seed, e, t, stream):
    """the four u of environment e at draw counter t on `stream` (0: environment, 1: policy)"""
    w = philox((e & _MASK, (e >> 32) & _MASK, t & _MASK, ((t >> 32) & 0xFFFFFF) | (stream << 24)),
               (seed & _MASK, (seed >> 32) & _MASK))
    return [((x >> 8) + 0.5) * 2.0 ** -24 for x in w]


# ---------------------------------------------------------------------------------------------------------- environment
def observation(s, cx, buffer_size=30.0, max_steps=100, nq=5):
    return np.array([s["buffer"] / buffer_size, min(s["bandwidth"] / 20, 1.0), s["battery"], s["last_quality"] / nq,
                     s["last_vmaf"] / 100, cx, s["step_count"] / max_steps], dtype=np.float32)


def reset(bw0, cx, buffer_size=30.0, max_steps=100, nq=5):
    s = dict(buffer=10.0, bandwidth=float(bw0), battery=1.0, last_quality=2, last_vmaf=70.0, step_count=0, total_rebuffer=0.0)
    return s, observation(s, cx, buffer_size, max_steps, nq)


def step(s, action, factor, cx, bitrates=BITRATES, segment_duration=4.0, buffer_size=30.0, max_steps=100, checks=None):
    """-> (state, obs, reward, terminated, truncated, info).  checks: a list that receives (buffer before clamping, battery)"""
    s = dict(s)
    nq = len(bitrates)
    q = int(action[0])
    enh = int(action[1]) / (ENH_LEVELS - 1)
    chunk = bitrates[q] * segment_duration
    download = chunk / (s["bandwidth"] * 1000)
    level = s["buffer"] - download
    rebuffer = max(0, -level)
    s["total_rebuffer"] += rebuffer
    level2 = max(0, level) + segment_duration
    s["buffer"] = min(level2, buffer_size)
    base = 50 + (q / nq) * 40
    s["last_vmaf"] = min(base + enh * 10, 100)
    cost = 0.01 + enh * 0.02
    s["battery"] = max(0, s["battery"] - cost)
    if checks is not None:
        checks.append((level, s["battery"]))
    reward = s["last_vmaf"] / 100 - rebuffer * 10 - abs(q - s["last_quality"]) * 0.1 + s["battery"] * 0.1
    s["last_quality"] = q
    s["step_count"] += 1
    s["bandwidth"] = min(max(s["bandwidth"] * factor, 0.5), 50.0)
    terminated = s["step_count"] >= max_steps
    truncated = s["battery"] <= 0
    info = dict(vmaf=float(s["last_vmaf"]), rebuffer=float(rebuffer), bandwidth=float(s["bandwidth"]), buffer=float(s["buffer"]))
    return s, observation(s, cx, buffer_size, max_steps, nq), float(reward), bool(terminated), bool(truncated), info


def vec_rollout(num_envs, actions, seed, max_steps, checks=None):
    """The vectorised environment: reset(), then actions (T, N, 2) with the same-step reset.  Returns dict of arrays: obs0 (N, 7),
    obs (T, N, 7) (the reset observation where done), reward (T, N), terminated / truncated (T, N), vmaf / rebuffer / bandwidth /
    buffer / episode_return (T, N) (values of the finished step)."""
    T = actions.shape[0]
    st, t, ret = [], [0] * num_envs, [0.0] * num_envs
    obs0 = np.zeros((num_envs, 7), np.float32)
    for e in range(num_envs):
        u = uniforms(seed, e, 0, 0)
        s, o = reset(2 + 13 * u[2], 0.3 + 0.5 * u[3], max_steps=max_steps)
        st.append(s)
        obs0[e] = o
        t[e] = 1
    out = dict(obs0=obs0, obs=np.zeros((T, num_envs, 7), np.float32), terminated=np.zeros((T, num_envs), bool),
               truncated=np.zeros((T, num_envs), bool))
    for k in ("reward", "vmaf", "rebuffer", "bandwidth", "buffer", "episode_return"):
        out[k] = np.zeros((T, num_envs), np.float64)
    for i in range(T):
        for e in range(num_envs):
            u = uniforms(seed, e, t[e], 0)
            t[e] += 1
            s, o, r, term, trunc, info = step(st[e], actions[i, e], 0.8 + 0.4 * u[0], 0.3 + 0.5 * u[1], max_steps=max_steps,
                                              checks=checks)
            ret[e] += r
            out["reward"][i, e], out["terminated"][i, e], out["truncated"][i, e] = r, term, trunc
            for k in ("vmaf", "rebuffer", "bandwidth", "buffer"):
                out[k][i, e] = info[k]
            out["episode_return"][i, e] = ret[e]
            if term or trunc:
                s, o = reset(2 + 13 * u[2], 0.3 + 0.5 * u[3], max_steps=max_steps)
                ret[e] = 0.0
            st[e] = s
            out["obs"][i, e] = o
    return out


# ---------------------------------------------------------------------------------------------------------- network and sampling
def mlp(state, obs, n_hidden, n_heads):
    """state: name -> array (features.{0,2,..}, policy_heads.i, value_head); obs (B, obs_dim) -> (B, sum(heads) + 1) float64"""
    h = np.asarray(obs, np.float64)
    for i in range(n_hidden):
        w, b = np.asarray(state[f"features.{2 * i}.weight"], np.float64), np.asarray(state[f"features.{2 * i}.bias"], np.float64)
        h = np.maximum(h @ w.T + b, 0.0)
    outs = []
    for i in range(n_heads):
        w, b = np.asarray(state[f"policy_heads.{i}.weight"], np.float64), np.asarray(state[f"policy_heads.{i}.bias"], np.float64)
        outs.append(h @ w.T + b)
    outs.append(h @ np.asarray(state["value_head.weight"], np.float64).T + np.asarray(state["value_head.bias"], np.float64))
    return np.concatenate(outs, axis=1)


def log_softmax(x):
    m = x.max(axis=-1, keepdims=True)
    return x - m - np.log(np.exp(x - m).sum(axis=-1, keepdims=True))


def head_slices(heads):
    off, out = 0, []
    for n in heads:
        out.append(slice(off, off + n))
        off += n
    return out


def sample(head_outputs, heads, u):
    """inverse CDF per head: head_outputs (B, P), u (B, len(heads)) -> (actions (B, heads), log_prob (B,), margin (B, heads)):
    margin is the distance of u to the nearest interior CDF boundary"""
    x = np.asarray(head_outputs, np.float64)
    B = x.shape[0]
    acts = np.zeros((B, len(heads)), np.int64)
    logp = np.zeros(B)
    margin = np.ones((B, len(heads)))
    for j, sl in enumerate(head_slices(heads)):
        lp = log_softmax(x[:, sl])
        cdf = np.cumsum(np.exp(lp), axis=1)
        for b in range(B):
            k = 0
            while k < heads[j] - 1 and not u[b, j] < cdf[b, k]:
                k += 1
            acts[b, j] = k
            logp[b] += lp[b, k]
            margin[b, j] = np.abs(cdf[b, :-1] - u[b, j]).min()
    return acts, logp, margin


def log_prob_of(head_outputs, heads, actions):
    x = np.asarray(head_outputs, np.float64)
    out = np.zeros(x.shape[0])
    for j, sl in enumerate(head_slices(heads)):
        out += np.take_along_axis(log_softmax(x[:, sl]), np.asarray(actions)[:, j:j + 1].astype(np.int64), axis=1)[:, 0]
    return out


# ---------------------------------------------------------------------------------------------------------- GAE and the loss
def gae(rewards, values, dones, last_values, gamma, lam):
    """(T, N) arrays, last_values (N,) -> (returns, advantages) in float64"""
    r, v, d = (np.asarray(a, np.float64) for a in (rewards, values, dones))
    T = r.shape[0]
    adv = np.zeros_like(r)
    g = np.zeros(r.shape[1])
    nxt = np.asarray(last_values, np.float64)
    for t in range(T - 1, -1, -1):
        delta = r[t] + gamma * nxt * (1 - d[t]) - v[t]
        g = delta + gamma * lam * (1 - d[t]) * g
        adv[t] = g
        nxt = v[t]
    return adv + v, adv


def ppo_loss(head_outputs, heads, actions, old_log_probs, advantages, returns, clip_ratio, value_coef, entropy_coef):
    """float64 torch: -> (loss tensor attached to x, x (leaf, requires grad), stats dict of floats, ratio)"""
    x = torch.as_tensor(np.asarray(head_outputs), dtype=torch.float64).clone().requires_grad_(True)
    a = torch.as_tensor(np.asarray(actions), dtype=torch.int64)
    old = torch.as_tensor(np.asarray(old_log_probs), dtype=torch.float64)
    adv = torch.as_tensor(np.asarray(advantages), dtype=torch.float64)
    ret = torch.as_tensor(np.asarray(returns), dtype=torch.float64)
    adv = (adv - adv.mean()) / (adv.std() + 1e-8)
    new, ent = 0, 0
    for j, sl in enumerate(head_slices(heads)):
        lp = torch.log_softmax(x[:, sl], dim=-1)
        new = new + lp.gather(1, a[:, j:j + 1])[:, 0]
        ent = ent + (-(lp.exp() * lp).sum(-1)).mean()
    ratio = (new - old).exp()
    s1, s2 = ratio * adv, torch.clamp(ratio, 1 - clip_ratio, 1 + clip_ratio) * adv
    pol = -torch.min(s1, s2).mean()
    val = ((x[:, -1] - ret) ** 2).mean()
    loss = pol + value_coef * val - entropy_coef * ent
    with torch.no_grad():
        lr = new - old
        stats = dict(loss=loss.item(), policy_loss=pol.item(), value_loss=val.item(), entropy=ent.item(),
                     approx_kl=((ratio - 1) - lr).mean().item(),
                     clip_fraction=((ratio - 1).abs() > clip_ratio).double().mean().item())
    return loss, x, stats, ratio.detach()
