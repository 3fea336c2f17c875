"""PPO agent for adaptive bitrate and enhancement-strength control (reference nerve_cl/abr/agent.py).

``ActorCritic`` keeps the reference's state-dict keys (``features.{0,2,..}``, ``policy_heads.i``, ``value_head``) and forward;
``PPOAgent`` keeps ``select_action`` / ``store_transition`` / ``update`` / ``save`` / ``load`` over one environment's stream, so a
checkpoint moves both ways.  That single-stream mode is a thin layer over the package's own pieces: ``select_action`` is ``act`` on a
batch of one with the agent's own draw counter, ``update`` is ``gae_stream`` (float64 on the host, bootstrap 0 as the reference
has it) followed by the same epoch loop as the vectorised mode; on the CPU its loss is ``ops.ppo_loss_composition`` in fp32, whose
operations are those of ``torch.distributions.Categorical``, so the numbers are the reference's.  New: ``ActorCritic.act`` (forward and sampling in one launch, nvq_abr_act) and
``PPOAgent.collect(vec_env, T)``, after which ``update()`` consumes the device rollout: one GAE launch, the advantage statistics as
a device reduction, ``ppo_epochs`` full-batch passes whose forward and backward are torch (``F.linear`` and autograd are plumbing
around rocBLAS GEMMs) ending in the fused ``ops.ppo_loss`` node, ``ops.clip_grad_norm_`` and the Adam step.

Differences from the reference: ``ABRConfig`` gains ``ppo_epochs`` (10) and ``max_grad_norm`` (0.5), the two constants its
``update()`` hard-codes; ``update()`` also returns ``policy_loss``, ``value_loss``, ``entropy``, ``approx_kl`` and
``clip_fraction`` of the last epoch; ``select_action`` samples from the agent's Philox stream (``seed``), not from torch's global
generator; ``load`` maps the checkpoint onto the agent's device."""
from __future__ import annotations

import warnings
from dataclasses import dataclass
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch
import torch.nn as nn

from nerve_cl import _nvq, ops
from nerve_cl.abr.environment import STREAM_POLICY, VecStreamingEnv


@dataclass
class ABRConfig:
    """Hyper-parameters of PPOAgent; the first seven fields and their defaults are the reference's."""
    hidden_dims: Tuple[int, ...] = (256, 256)
    learning_rate: float = 3e-4
    gamma: float = 0.99
    gae_lambda: float = 0.95
    clip_ratio: float = 0.2
    value_coef: float = 0.5
    entropy_coef: float = 0.01
    ppo_epochs: int = 10
    max_grad_norm: float = 0.5


def philox_uniforms(env: torch.Tensor, t: torch.Tensor, stream: int, seed: int) -> torch.Tensor:
    """(B, 4) float64 u of (environment, draw counter) on `stream` in torch integer arithmetic on the tensors' device: the rule of
    include/nvq.h ("ABR agent").  The 32 x 32 products wrap in int64; their bit patterns are the unsigned ones."""
    m = 0xFFFFFFFF
    c0, c1, c2 = env & m, (env >> 32) & m, t & m
    c3 = ((t >> 32) & 0xFFFFFF) | (stream << 24)
    k0, k1 = seed & m, (seed >> 32) & m
    for _ in range(10):
        p0, p1 = c0 * 0xD2511F53, c2 * 0xCD9E8D57
        c0, c1, c2, c3 = ((p1 >> 32) & m) ^ c1 ^ k0, p1 & m, ((p0 >> 32) & m) ^ c3 ^ k1, p0 & m
        k0, k1 = (k0 + 0x9E3779B9) & m, (k1 + 0xBB67AE85) & m
    w = torch.stack([c0, c1, c2, c3], dim=-1)
    return ((w >> 8).double() + 0.5) * 2.0 ** -24


def gae_stream(rewards: Sequence[float], values: Sequence[float], dones: Sequence[bool], gamma: float, lam: float,
               last_value: float = 0.0) -> Tuple[np.ndarray, np.ndarray]:
    """Generalised advantage estimation over one stream in float64 -> (returns, advantages).  Backwards from the last step:
    delta_t = r_t + gamma v_(t+1) (1 - d_t) - v_t, A_t = delta_t + gamma lam (1 - d_t) A_(t+1), return_t = A_t + v_t, with
    v_T = ``last_value``.  Products are taken left to right, which fixes the rounding."""
    n = len(rewards)
    adv, ret = np.zeros(n, dtype=np.float64), np.zeros(n, dtype=np.float64)
    running, v_next = 0.0, float(last_value)
    for t in range(n - 1, -1, -1):
        keep = 1 - int(bool(dones[t]))
        v = float(values[t])
        delta = float(rewards[t]) + gamma * v_next * keep - v
        running = delta + gamma * lam * keep * running
        adv[t], ret[t] = running, running + v
        v_next = v
    return ret, adv


class ActorCritic(nn.Module):
    """Shared ReLU MLP ``features`` (Linear at the even indices), one Linear per action dimension in ``policy_heads`` and a
    one-output ``value_head``; forward returns (logits_0, .., value)."""

    def __init__(self, obs_dim: int, num_actions: Sequence[int], hidden_dims: Sequence[int] = (256, 256)):
        super().__init__()
        self.obs_dim, self.num_actions = int(obs_dim), tuple(int(n) for n in num_actions)
        self.hidden_dims = tuple(int(w) for w in hidden_dims)
        widths = (self.obs_dim,) + self.hidden_dims
        self.features = nn.Sequential(*[m for i, o in zip(widths[:-1], widths[1:]) for m in (nn.Linear(i, o), nn.ReLU())])
        self.policy_heads = nn.ModuleList(nn.Linear(widths[-1], n) for n in self.num_actions)
        self.value_head = nn.Linear(widths[-1], 1)
        self._fused = None

    def forward(self, obs: torch.Tensor) -> Tuple[torch.Tensor, ...]:
        h = self.features(obs)
        return (*(head(h) for head in self.policy_heads), self.value_head(h))

    @property
    def fused(self) -> bool:
        """whether nvq_abr_act serves this network's shapes (fixed at construction, asked of the library once)"""
        if self._fused is None:
            self._fused = _nvq.abr_act_supported(self.obs_dim, self.hidden_dims, self.num_actions)
        return self._fused

    def head_outputs(self, obs: torch.Tensor) -> torch.Tensor:
        """(B, sum(heads) + 1): the heads' logits, then the value (the layout of ops.ppo_loss)"""
        return torch.cat(self.forward(obs), dim=-1)

    def _act_torch(self, obs, counters, seed, deterministic):
        """the rule of nvq_abr_act as a torch composition on the tensors' device"""
        x = self.head_outputs(obs)
        B = x.shape[0]
        u = None
        if not deterministic and counters is not None:
            u = philox_uniforms(torch.arange(B, dtype=torch.int64, device=x.device), counters, STREAM_POLICY, seed).float()
        acts, logp, off = [], 0, 0
        for j, n in enumerate(self.num_actions):
            lp = torch.log_softmax(x[:, off:off + n], dim=-1)
            if u is None:
                a = lp.argmax(dim=-1)
            else:
                a = (u[:, j:j + 1] >= lp.exp().cumsum(dim=-1)).sum(dim=-1).clamp(max=n - 1)
            logp = logp + lp.gather(1, a[:, None])[:, 0]
            acts.append(a)
            off += n
        return torch.stack(acts, dim=-1).int(), logp, x[:, -1].clone(), x

    @torch.no_grad()
    def act(self, obs: torch.Tensor, counters: Optional[torch.Tensor] = None, seed: int = 0, deterministic: bool = False,
            fused: Optional[bool] = None, out: Optional[tuple] = None, return_head_outputs: bool = False):
        """-> (actions int32 (B, heads), log_prob (B,), value (B,)).  Head j of row i samples by inverse CDF with word j of the
        Philox call (environment i, counters[i]) on the policy stream with key ``seed``; ``deterministic`` or no ``counters``:
        the first index of the maximum.  On HIP tensors and supported shapes (``self.fused``) this is one launch; otherwise the
        same rule as a torch composition (``fused=False`` forces it; ``fused=True`` raises where the kernel cannot serve).
        ``out``: (actions, log_prob, value) tensors to write, e.g. a rollout's rows."""
        B = obs.shape[0]
        use = obs.is_cuda and self.fused if fused is None else fused
        if use:
            if not (obs.is_cuda and self.fused):
                raise RuntimeError("ActorCritic.act: the fused kernel needs HIP tensors and a supported network (see nvq_abr_act)")
            obs = obs.detach().float().contiguous()
            if out is None:
                out = (torch.empty(B, len(self.num_actions), dtype=torch.int32, device=obs.device),
                       torch.empty(B, dtype=torch.float32, device=obs.device), torch.empty(B, dtype=torch.float32, device=obs.device))
            ho = torch.empty(B, sum(self.num_actions) + 1, dtype=torch.float32, device=obs.device) if return_head_outputs else None
            lin = [m for m in self.features if isinstance(m, nn.Linear)]
            with _nvq.device_guard(obs.device):
                _nvq.abr_act(obs, [(m.weight, m.bias) for m in lin], [(m.weight, m.bias) for m in self.policy_heads],
                             (self.value_head.weight, self.value_head.bias), counters, seed, deterministic, *out, ho)
            return (*out, ho) if return_head_outputs else out
        a, lp, v, x = self._act_torch(obs.float(), counters, seed, deterministic)
        if out is not None:
            out[0].copy_(a)
            out[1].copy_(lp)
            out[2].copy_(v)
            a, lp, v = out
        return (a, lp, v, x) if return_head_outputs else (a, lp, v)


class PPOAgent:
    """PPO for the streaming environment: the single-stream surface of the reference and the vectorised collect / update."""

    BUFFER_KEYS = ("obs", "actions", "rewards", "values", "log_probs", "dones")

    def __init__(self, obs_dim: int, num_actions: Sequence[int], config: Optional[ABRConfig] = None, device="cpu",
                 fused: Optional[bool] = None, seed: int = 0):
        self.config = ABRConfig() if config is None else config
        self.device = device
        dev = torch.device(device)
        self.network = ActorCritic(obs_dim, num_actions, self.config.hidden_dims).to(dev)
        self.optimizer = torch.optim.Adam(self.network.parameters(), lr=self.config.learning_rate)
        self.buffer = {k: [] for k in self.BUFFER_KEYS}
        self.seed = int(seed)
        self._draws = torch.zeros(1, dtype=torch.int64, device=dev)       # draw counter of the single stream
        served = dev.type == "cuda" and self.network.fused
        if fused and not served:
            raise RuntimeError("PPOAgent: fused=True needs a HIP device and a network nvq_abr_act serves")
        self._fused = served if fused is None else bool(fused)
        if dev.type == "cuda" and fused is None and not served:
            warnings.warn(f"PPOAgent: nvq_abr_act does not serve obs_dim {obs_dim}, hidden {tuple(self.config.hidden_dims)}, heads "
                          f"{tuple(num_actions)} (obs_dim <= 32, 1 to 3 hidden layers of a multiple of 32 in [32, 512], at most 4 heads "
                          "and 32 head outputs with the value): collect() acts through the torch composition on the device",
                          stacklevel=2)
        self._rollout = None
        self._collected = False
        self._env = None

    @property
    def fused(self) -> bool:
        """whether ``collect`` acts through the fused kernel (False: the torch composition on the device)"""
        return self._fused

    # ------------------------------------------------------------------ single stream: one observation at a time
    def select_action(self, obs: np.ndarray, deterministic: bool = False) -> np.ndarray:
        """One decision for one observation.  Sampling is ``act`` on a batch of one with this agent's draw counter; the
        observation, log-probability and value are kept for ``update`` unless ``deterministic``."""
        row = torch.as_tensor(np.asarray(obs), dtype=torch.float32).reshape(1, -1).to(self._draws.device)
        if deterministic:
            return self.network.act(row, deterministic=True)[0][0].cpu().numpy()
        action, log_prob, value = self.network.act(row, self._draws, seed=self.seed)
        self._draws += 1
        kept = torch.stack([log_prob[0], value[0]]).tolist()
        self.buffer["obs"].append(obs)
        self.buffer["log_probs"].append(kept[0])
        self.buffer["values"].append(kept[1])
        return action[0].cpu().numpy()

    def store_transition(self, action: np.ndarray, reward: float, done: bool):
        for key, item in (("actions", action), ("rewards", reward), ("dones", done)):
            self.buffer[key].append(item)

    def _update_stream(self) -> Dict[str, float]:
        cfg, buf, dev = self.config, self.buffer, self._draws.device
        ret, adv = gae_stream(buf["rewards"], buf["values"], buf["dones"], cfg.gamma, cfg.gae_lambda)
        f32 = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.float32).to(dev)      # noqa: E731
        batch = (f32(np.stack(buf["obs"])), torch.as_tensor(np.stack(buf["actions"]), dtype=torch.int32).to(dev), f32(buf["log_probs"]),
                 f32(adv), f32(ret))
        self.buffer = {k: [] for k in self.BUFFER_KEYS}
        return self._epochs(*batch, None, exact_fp32=dev.type != "cuda")

    # ------------------------------------------------------------------ vectorised rollouts
    def collect(self, vec_env: VecStreamingEnv, num_steps: int) -> dict:
        """``num_steps`` steps of every environment: per step one act launch and one environment launch, stored into a preallocated
        (T, N, ...) rollout on the environment's device, then the bootstrap value of the final observation.  No host
        synchronisation; nothing passed by value changes from step to step, so a whole collect can be captured in a graph.
        Returns the rollout (tensors that the next collect overwrites)."""
        T, N, dev = int(num_steps), vec_env.num_envs, vec_env.state.device
        if dev != next(self.network.parameters()).device:
            raise RuntimeError(f"PPOAgent.collect: the environment lives on {dev}, the network on {next(self.network.parameters()).device}")
        nh, od = len(self.network.num_actions), self.network.obs_dim
        ro = self._rollout
        if ro is None or ro["rewards"].shape != (T, N) or ro["rewards"].device != dev:
            f32 = dict(dtype=torch.float32, device=dev)
            ro = self._rollout = dict(
                obs=torch.zeros(T + 1, N, od, **f32), actions=torch.zeros(T, N, nh, dtype=torch.int32, device=dev),
                log_probs=torch.zeros(T, N, **f32), values=torch.zeros(T, N, **f32), rewards=torch.zeros(T, N, **f32),
                dones=torch.zeros(T, N, **f32), last_values=torch.zeros(N, **f32), returns=torch.zeros(T, N, **f32),
                advantages=torch.zeros(T, N, **f32), reward64=torch.zeros(N, dtype=torch.float64, device=dev),
                terminated=torch.zeros(T, N, dtype=torch.bool, device=dev), truncated=torch.zeros(T, N, dtype=torch.bool, device=dev),
                scratch_actions=torch.zeros(N, nh, dtype=torch.int32, device=dev), scratch_lp=torch.zeros(N, **f32))
        ro["obs"][0].copy_(vec_env.obs)
        for t in range(T):
            self.network.act(ro["obs"][t], vec_env.counters, vec_env.seed, fused=self._fused,
                             out=(ro["actions"][t], ro["log_probs"][t], ro["values"][t]))
            vec_env.step_into(ro["actions"][t], ro["obs"][t + 1], ro["reward64"], ro["terminated"][t], ro["truncated"][t],
                              reward_f32=ro["rewards"][t], done_f32=ro["dones"][t])
        self.network.act(ro["obs"][T], None, 0, deterministic=True, fused=self._fused,
                         out=(ro["scratch_actions"], ro["scratch_lp"], ro["last_values"]))
        self._collected, self._env = True, vec_env
        return ro

    def _epochs(self, obs, actions, old, adv, ret, stats, exact_fp32: bool = False, extra: Optional[torch.Tensor] = None):
        """``ppo_epochs`` full-batch passes: forward, loss, backward, clipping, Adam; the metrics (and ``extra``) come back in one
        host copy after the last.  ``exact_fp32``: the fp32 composition of the loss (the single stream on the CPU)."""
        cfg, heads = self.config, self.network.num_actions
        total, last = 0.0, None
        for _ in range(cfg.ppo_epochs):
            if exact_fp32:
                loss, last = ops.ppo_loss_composition(self.network(obs), heads, actions, old, adv, ret, cfg.clip_ratio, cfg.value_coef,
                                                      cfg.entropy_coef, stats, dtype=torch.float32)
            else:
                loss, last = ops.ppo_loss(self.network(obs), actions, old, adv, ret, cfg.clip_ratio, cfg.value_coef, cfg.entropy_coef,
                                          adv_stats=stats, return_stats=True)
            self.optimizer.zero_grad()
            loss.backward()
            ops.clip_grad_norm_(self.network, cfg.max_grad_norm)
            self.optimizer.step()
            total = total + last[0].double()
        parts = [total.reshape(1) / cfg.ppo_epochs, last.double()] + ([] if extra is None else [extra.double().reshape(-1)])
        host = torch.cat(parts).cpu().tolist()                                     # the one read-back
        names = ("loss", "last_loss", "policy_loss", "value_loss", "entropy", "approx_kl", "clip_fraction")
        out = dict(zip(names, host))
        if extra is not None:
            out["episode_return_sum"], out["episodes_finished"] = host[len(names):]
        return out

    def _update_rollout(self) -> Dict[str, float]:
        cfg, ro = self.config, self._rollout
        T, N = ro["rewards"].shape
        dev = ro["rewards"].device
        stats = None
        if dev.type == "cuda":
            stats = torch.empty(2, dtype=torch.float64, device=dev)
            with _nvq.device_guard(dev):
                _nvq.abr_gae(ro["rewards"], ro["values"], ro["dones"], ro["last_values"], cfg.gamma, cfg.gae_lambda, ro["returns"],
                             ro["advantages"])
                _nvq.abr_adv_stats(ro["advantages"], stats)
        else:
            gae, nxt = torch.zeros(N), ro["last_values"]
            for t in range(T - 1, -1, -1):
                nd = 1.0 - ro["dones"][t]
                delta = ro["rewards"][t] + cfg.gamma * nxt * nd - ro["values"][t]
                gae = delta + cfg.gamma * cfg.gae_lambda * nd * gae
                ro["advantages"][t], ro["returns"][t] = gae, gae + ro["values"][t]
                nxt = ro["values"][t]
        self._collected = False
        return self._epochs(ro["obs"][:T].reshape(T * N, -1), ro["actions"].reshape(T * N, -1), ro["log_probs"].reshape(-1),
                            ro["advantages"].reshape(-1), ro["returns"].reshape(-1), stats, extra=self._env.finished.sum(dim=0))

    def update(self) -> Dict[str, float]:
        """The PPO update on the rollout of the last ``collect`` when there is one, else on the single-stream buffer.  Returns
        ``loss`` (the mean over the epochs) and the last epoch's ``policy_loss``, ``value_loss``, ``entropy``, ``approx_kl`` and
        ``clip_fraction``; after a ``collect`` also the environments' running totals ``episode_return_sum`` and
        ``episodes_finished``, all from one host copy."""
        return self._update_rollout() if self._collected else self._update_stream()

    # ------------------------------------------------------------------ checkpoints: {"network", "optimizer"} state dicts
    def save(self, path: str):
        state = {"network": self.network.state_dict(), "optimizer": self.optimizer.state_dict()}
        torch.save(state, path)

    def load(self, path: str):
        state = torch.load(path, map_location=self._draws.device)
        for name, target in (("network", self.network), ("optimizer", self.optimizer)):
            target.load_state_dict(state[name])
