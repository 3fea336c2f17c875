"""The streaming environment of the ABR agent (reference nerve_cl/abr/environment.py): one environment on the host with the
reference's surface, and the same environment N times on the device (csrc/abr.hip).

State [buffer level, bandwidth, battery, last quality, last VMAF, step count, total rebuffer]; observation = the reference's
7-vector as float32; action (bitrate index, enhancement level); reward = quality - rebuffer penalty - smoothness penalty + battery
bonus.  All arithmetic is float64 in the reference's order of operations; the rule is written once for the host (``_Rule``, numpy
rows) and once for the device (csrc/abr.hip), and recorded reference episodes (tests/golden) pin both.

Differences from the reference
  * ``gymnasium`` is not needed: ``action_space`` / ``observation_space`` are minimal stand-ins (``sample()``, ``shape``, ``nvec``,
    ``dtype``).
  * ``StreamingEnv`` draws from a ``numpy.random.Generator`` it owns, reseeded by ``reset(seed=)``; the reference draws from
    numpy's global state (``np.random.uniform``), which ``reset(seed=)`` does not touch.  The draws are the same four: bandwidth
    U(2, 15) and content complexity U(0.3, 0.8) per reset, bandwidth factor U(0.8, 1.2) and complexity per step.
  * ``VecStreamingEnv`` draws from Philox4x32-10 keyed by ``seed`` with the counter (environment, draw counter, stream 0): word 0
    is the bandwidth factor 0.8 + 0.4 u, word 1 the complexity 0.3 + 0.5 u of the returned observation, word 2 the reset
    bandwidth 2 + 13 u and word 3 the reset observation's complexity (include/nvq.h, "ABR agent").  The draw counter advances by
    one per ``step`` and per ``reset`` call for every environment, so a rollout is a function of (seed, actions) alone.
  * ``VecStreamingEnv.step`` resets an environment that finishes INSIDE the same step: reward, flags and ``info`` are those of the
    finished step, the returned observation is already the reset observation of the next episode; the flags tell the caller.
    Nothing returns to the host.  Actions outside their range are clamped into it.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from nerve_cl import _nvq
from nerve_cl.federated._philox import philox4x32_10

ENHANCEMENT_LEVELS = 5       # 0.0, 0.25, 0.5, 0.75, 1.0
OBS_DIM = 7
STREAM_ENV, STREAM_POLICY = 0, 1


@dataclass
class QualityLevel:
    """One rung of the bitrate ladder."""
    resolution: int   # lines, 360 to 1440 in the default ladder
    bitrate: int      # kbit/s


def default_ladder() -> List[QualityLevel]:
    return [QualityLevel(360, 365), QualityLevel(480, 750), QualityLevel(720, 1500), QualityLevel(1080, 3000),
            QualityLevel(1440, 6000)]


class MultiDiscreteSpace:
    """stand-in for gymnasium.spaces.MultiDiscrete"""

    def __init__(self, nvec, seed: Optional[int] = None):
        self.nvec = np.asarray(nvec, dtype=np.int64)
        self.shape = self.nvec.shape
        self.dtype = np.int64
        self._rng = np.random.default_rng(seed)

    def sample(self) -> np.ndarray:
        return (self._rng.random(self.nvec.shape) * self.nvec).astype(self.dtype)


class BoxSpace:
    """stand-in for gymnasium.spaces.Box"""

    def __init__(self, low: float, high: float, shape: Tuple[int, ...], dtype=np.float32, seed: Optional[int] = None):
        self.low, self.high, self.shape, self.dtype = low, high, tuple(shape), dtype
        self._rng = np.random.default_rng(seed)

    def sample(self) -> np.ndarray:
        return self._rng.uniform(self.low, self.high, self.shape).astype(self.dtype)


class _Rule:
    """The transition on (n, 8) float64 numpy state rows {buffer, bandwidth, battery, last quality, last VMAF, step count, total
    rebuffer, episode return}: what csrc/abr.hip computes per thread, shared by StreamingEnv (n = 1) and VecStreamingEnv's CPU
    route.  Every expression is evaluated left to right in float64, which fixes the rounding."""

    def __init__(self, bitrates: List[int], segment_duration: float, buffer_size: float, max_steps: int, levels: int):
        self.kbps = np.asarray(bitrates, dtype=np.float64)
        self.seg, self.cap, self.max_steps, self.levels = float(segment_duration), float(buffer_size), int(max_steps), int(levels)

    def observe(self, s: np.ndarray, cx: np.ndarray) -> np.ndarray:
        cols = [s[:, 0] / self.cap, np.minimum(s[:, 1] / 20, 1.0), s[:, 2], s[:, 3] / len(self.kbps), s[:, 4] / 100, cx,
                s[:, 5] / self.max_steps]
        return np.stack(cols, axis=1).astype(np.float32)

    @staticmethod
    def start(s: np.ndarray, rows: np.ndarray, bandwidth: np.ndarray) -> None:
        """rows begin an episode: 10 s buffered, full battery, the middle quality (720p) at VMAF 70"""
        s[rows] = 0.0
        s[rows, 0], s[rows, 1], s[rows, 2], s[rows, 3], s[rows, 4] = 10.0, bandwidth, 1.0, 2.0, 70.0

    def advance(self, s: np.ndarray, actions: np.ndarray, factor: np.ndarray):
        """one segment per row, in place -> (reward, rebuffer, terminated, truncated); actions are clamped into range"""
        q = np.clip(actions[:, 0], 0, len(self.kbps) - 1).astype(np.int64)
        strength = np.clip(actions[:, 1], 0, self.levels - 1).astype(np.float64) / (self.levels - 1)
        level = s[:, 0] - self.kbps[q] * self.seg / (s[:, 1] * 1000)         # kbit over kbit/s: the download drains the buffer
        stall = np.maximum(0.0, -level)
        s[:, 6] = s[:, 6] + stall
        s[:, 0] = np.minimum(np.maximum(0.0, level) + self.seg, self.cap)
        s[:, 4] = np.minimum(50 + (q / len(self.kbps)) * 40 + strength * 10, 100.0)
        s[:, 2] = np.maximum(0.0, s[:, 2] - (0.01 + strength * 0.02))
        reward = s[:, 4] / 100 - stall * 10 - np.abs(q - s[:, 3].astype(np.int64)) * 0.1 + s[:, 2] * 0.1
        s[:, 3] = q
        s[:, 5] = s[:, 5] + 1
        s[:, 1] = np.minimum(np.maximum(s[:, 1] * factor, 0.5), 50.0)
        s[:, 7] = s[:, 7] + reward
        return reward, stall, s[:, 5] >= self.max_steps, s[:, 2] <= 0


class StreamingEnv:
    """One environment on the host with the reference's surface: ``reset(seed=None, options=None) -> (obs, {})`` and
    ``step(action) -> (obs, reward, terminated, truncated, info)`` with ``info`` keys vmaf / rebuffer / bandwidth / buffer.  It is
    one row of ``_Rule`` fed from ``np_random``."""

    metadata = {"render_modes": ["human"]}

    def __init__(self, quality_ladder: Optional[List[QualityLevel]] = None, segment_duration: float = 4.0, buffer_size: float = 30.0,
                 max_steps: int = 100):
        self.quality_ladder = list(quality_ladder) if quality_ladder else default_ladder()
        self.segment_duration, self.buffer_size, self.max_steps = segment_duration, buffer_size, max_steps
        self.num_qualities, self.enhancement_levels = len(self.quality_ladder), ENHANCEMENT_LEVELS
        self._rule = _Rule([q.bitrate for q in self.quality_ladder], segment_duration, buffer_size, max_steps, ENHANCEMENT_LEVELS)
        self._s = np.zeros((1, 8), dtype=np.float64)
        self.action_space = MultiDiscreteSpace([self.num_qualities, self.enhancement_levels])
        self.observation_space = BoxSpace(0.0, 1.0, (OBS_DIM,), np.float32)
        self.np_random = np.random.default_rng()
        self.reset()

    def _draw(self, low: float, high: float) -> np.ndarray:
        return np.array([self.np_random.uniform(low, high)], dtype=np.float64)

    def reset(self, seed: Optional[int] = None, options: Optional[dict] = None) -> Tuple[np.ndarray, dict]:
        if seed is not None:
            self.np_random = np.random.default_rng(seed)
        self._rule.start(self._s, np.array([0]), self._draw(2, 15))
        return self._rule.observe(self._s, self._draw(0.3, 0.8))[0], {}

    def step(self, action) -> Tuple[np.ndarray, float, bool, bool, dict]:
        if not 0 <= int(action[0]) < self.num_qualities:
            raise IndexError(f"StreamingEnv.step: quality index {int(action[0])} outside the ladder")
        reward, stall, term, trunc = self._rule.advance(self._s, np.asarray(action).reshape(1, 2), self._draw(0.8, 1.2))
        s = self._s[0]
        info = {"vmaf": float(s[4]), "rebuffer": float(stall[0]), "bandwidth": float(s[1]), "buffer": float(s[0])}
        return self._rule.observe(self._s, self._draw(0.3, 0.8))[0], float(reward[0]), bool(term[0]), bool(trunc[0]), info


def make_env(env_id: str = "Streaming-v0", **kwargs) -> StreamingEnv:
    return StreamingEnv(**kwargs)


def host_uniforms(seed: int, env: np.ndarray, t: np.ndarray, stream: int) -> np.ndarray:
    """(n, 4) float64 u of (environment, draw counter) pairs on `stream`: the host twin of abr_words in csrc/abr.hip"""
    env, t = np.asarray(env, dtype=np.uint64), np.asarray(t, dtype=np.uint64)
    m = np.uint64(0xFFFFFFFF)
    ctr = np.stack([env & m, env >> np.uint64(32), t & m, ((t >> np.uint64(32)) & np.uint64(0xFFFFFF)) | np.uint64(stream << 24)],
                   axis=-1)
    key = np.broadcast_to(np.array([seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF], dtype=np.uint64), (len(env), 2))
    w = philox4x32_10(ctr, key)
    return ((w >> np.uint32(8)).astype(np.float64) + 0.5) * 2.0 ** -24


class VecStreamingEnv:
    """``num_envs`` streaming environments stepped together.  On a HIP device the state is an (N, 8) float64 tensor {buffer,
    bandwidth, battery, last quality, last VMAF, step count, total rebuffer, episode return} plus the (N,) int64 draw counters
    ``counters``, and ``reset`` / ``step`` are one launch each without a host synchronisation; on the CPU the same rule runs in
    float64 numpy with the host Philox.  ``obs`` is the current observation (N, 7) float32; ``finished`` (N, 2) float64 holds
    each environment's sum of finished episode returns and their count."""

    def __init__(self, num_envs: int, quality_ladder: Optional[List[QualityLevel]] = None, segment_duration: float = 4.0,
                 buffer_size: float = 30.0, max_steps: int = 100, seed: int = 0, device="cuda"):
        if num_envs < 1 or seed < 0:
            raise ValueError("VecStreamingEnv: num_envs >= 1 and seed >= 0")
        self.num_envs = int(num_envs)
        self.quality_ladder = quality_ladder or default_ladder()
        self.bitrates = [int(q.bitrate) for q in self.quality_ladder]
        if not 1 <= len(self.bitrates) <= 16:
            raise ValueError("VecStreamingEnv: 1 to 16 quality levels")
        self.segment_duration, self.buffer_size, self.max_steps = float(segment_duration), float(buffer_size), int(max_steps)
        self.num_qualities, self.enhancement_levels = len(self.bitrates), ENHANCEMENT_LEVELS
        self.seed = int(seed)
        self.device = torch.device(device)
        self.action_space = MultiDiscreteSpace([self.num_qualities, self.enhancement_levels])
        self.observation_space = BoxSpace(0.0, 1.0, (OBS_DIM,), np.float32)
        N, dev = self.num_envs, self.device
        self.state = torch.zeros(N, 8, dtype=torch.float64, device=dev)
        self.counters = torch.zeros(N, dtype=torch.int64, device=dev)
        self.obs = torch.zeros(N, OBS_DIM, dtype=torch.float32, device=dev)
        self.finished = torch.zeros(N, 2, dtype=torch.float64, device=dev)
        self._params = torch.tensor([self.segment_duration, self.buffer_size], dtype=torch.float64, device=dev)
        self._rule = _Rule(self.bitrates, self.segment_duration, self.buffer_size, self.max_steps, self.enhancement_levels)
        self.reset()

    # ------------------------------------------------------------------ the rule on the host (CPU tensors)
    def _reset_cpu(self) -> None:
        s, t = self.state.numpy(), self.counters.numpy()
        u = host_uniforms(self.seed, np.arange(self.num_envs), t, STREAM_ENV)
        self._rule.start(s, np.arange(self.num_envs), 2 + 13 * u[:, 2])
        self.obs.copy_(torch.from_numpy(self._rule.observe(s, 0.3 + 0.5 * u[:, 3])))
        t += 1

    def _step_cpu(self, actions: torch.Tensor, obs, reward, terminated, truncated, info, reward_f32, done_f32) -> None:
        s, t = self.state.numpy(), self.counters.numpy()
        u = host_uniforms(self.seed, np.arange(self.num_envs), t, STREAM_ENV)
        rew, stall, term, trunc = self._rule.advance(s, actions.numpy(), 0.8 + 0.4 * u[:, 0])
        done = term | trunc
        reward.copy_(torch.from_numpy(rew))
        terminated.copy_(torch.from_numpy(term))
        truncated.copy_(torch.from_numpy(trunc))
        if info is not None:
            info.copy_(torch.from_numpy(np.stack([s[:, 4], stall, s[:, 1], s[:, 0], s[:, 7]])))
        if reward_f32 is not None:
            reward_f32.copy_(torch.from_numpy(rew.astype(np.float32)))
        if done_f32 is not None:
            done_f32.copy_(torch.from_numpy(done.astype(np.float32)))
        cx = 0.3 + 0.5 * u[:, 1]
        rows = np.nonzero(done)[0]
        if rows.size:
            fin = self.finished.numpy()
            fin[rows, 0] += s[rows, 7]
            fin[rows, 1] += 1
            self._rule.start(s, rows, 2 + 13 * u[rows, 2])
            cx[rows] = 0.3 + 0.5 * u[rows, 3]
        obs.copy_(torch.from_numpy(self._rule.observe(s, cx)))
        t += 1

    # ------------------------------------------------------------------ public surface
    def reset(self, seed: Optional[int] = None, options: Optional[dict] = None) -> torch.Tensor:
        """Start a new episode in every environment; returns obs (N, 7) float32.  ``seed``: a new Philox key, draw counters to 0."""
        if seed is not None:
            if seed < 0:
                raise ValueError("VecStreamingEnv: seed >= 0")
            self.seed = int(seed)
            self.counters.zero_()
        if self.device.type == "cuda":
            with _nvq.device_guard(self.device):
                _nvq.abr_env_reset(self.state, self.counters, self.obs, self._params, self.num_qualities, self.max_steps, self.seed)
        else:
            self._reset_cpu()
        return self.obs.clone()

    def step_into(self, actions: torch.Tensor, obs: torch.Tensor, reward: torch.Tensor, terminated: torch.Tensor,
                  truncated: torch.Tensor, info: Optional[torch.Tensor] = None, reward_f32: Optional[torch.Tensor] = None,
                  done_f32: Optional[torch.Tensor] = None) -> None:
        """``step`` into tensors of the caller (a rollout's rows): obs (N, 7) f32, reward (N,) f64, flags (N,) bool, info (5, N)
        f64 {vmaf, rebuffer, bandwidth, buffer, episode_return}, reward_f32 / done_f32 (N,) f32.  ``self.obs`` becomes ``obs``."""
        if actions.dtype != torch.int32 or tuple(actions.shape) != (self.num_envs, 2) or actions.device != self.state.device:
            raise RuntimeError(f"VecStreamingEnv.step: actions must be ({self.num_envs}, 2) int32 on {self.state.device}")
        if self.device.type == "cuda":
            with _nvq.device_guard(self.device):
                _nvq.abr_env_step(self.state, self.counters, actions.contiguous(), self.bitrates, self.enhancement_levels,
                                  self.max_steps, self._params, self.seed, obs, reward, terminated, truncated, info, reward_f32,
                                  done_f32, self.finished)
        else:
            self._step_cpu(actions, obs, reward, terminated, truncated, info, reward_f32, done_f32)
        self.obs = obs

    def step(self, actions: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, Dict[str, torch.Tensor]]:
        """actions (N, 2) int32 -> (obs (N, 7) f32, reward (N,) f64, terminated, truncated (N,) bool, info) as tensors on the
        environment's device.  A finished environment is reset inside this step (see the module docstring)."""
        N, dev = self.num_envs, self.state.device
        obs = torch.empty(N, OBS_DIM, dtype=torch.float32, device=dev)
        reward = torch.empty(N, dtype=torch.float64, device=dev)
        terminated = torch.empty(N, dtype=torch.bool, device=dev)
        truncated = torch.empty(N, dtype=torch.bool, device=dev)
        info = torch.empty(5, N, dtype=torch.float64, device=dev)
        self.step_into(actions, obs, reward, terminated, truncated, info)
        names = ("vmaf", "rebuffer", "bandwidth", "buffer", "episode_return")
        return obs, reward, terminated, truncated, {k: info[i] for i, k in enumerate(names)}
