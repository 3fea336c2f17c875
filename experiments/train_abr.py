#!/usr/bin/env python3
"""ABR agent training and evaluation with the command line of the reference's experiments/train_abr.py (``--mode``,
``--num-steps``, ``--learning-rate``, ``--device``, ``--model-path``) plus ``--num-envs N``, ``--rollout-steps T`` and ``--seed``.

``--device cpu --num-envs 1`` is the reference's schedule: one StreamingEnv on the host, one decision per step, an update when an
episode ends with at least 64 transitions held, a checkpoint whenever the mean of the last ten episode returns improves.  Any
other combination keeps N environments on the device (nerve_cl.abr.VecStreamingEnv) and alternates ``collect`` (T steps of all N:
one act launch and one environment launch per step, nothing returns to the host) with ``update`` (GAE, advantage statistics and
the fused PPO loss); ``--num-steps`` then counts environment steps, N * T per iteration.  The returns of finished episodes are
summed by the environments on the device and come back inside update()'s metrics: one host copy per update."""
import argparse
import statistics
from pathlib import Path

import _common  # noqa: F401
import torch

from nerve_cl.abr import ABRConfig, PPOAgent, StreamingEnv, VecStreamingEnv

CKPT_DIR = Path("checkpoints")
MIN_TRANSITIONS, REPORT_EVERY = 64, 10


def new_agent(args) -> PPOAgent:
    cfg = ABRConfig(learning_rate=args.learning_rate)
    return PPOAgent(7, (5, 5), cfg, device=args.device, seed=args.seed)


def episodes(env: StreamingEnv, agent: PPOAgent, budget: int, greedy: bool, seed=None):
    """yield (return, last info) per finished episode until `budget` steps are spent (None: forever); records transitions
    unless greedy"""
    obs, _ = env.reset(seed=seed)
    spent, total = 0, 0.0
    while budget is None or spent < budget:
        action = agent.select_action(obs, deterministic=greedy)
        obs, reward, terminated, truncated, info = env.step(action)
        over = terminated or truncated
        if not greedy:
            agent.store_transition(action, reward, over)
        spent, total = spent + 1, total + reward
        if over:
            yield total, info
            total = 0.0
            obs, _ = env.reset()


def train_host(args) -> None:
    agent = new_agent(args)
    print(f"single environment on the host, {args.num_steps} steps")
    returns, best = [], float("-inf")
    for ep_return, _ in episodes(StreamingEnv(max_steps=100), agent, args.num_steps, greedy=False, seed=args.seed):
        returns.append(ep_return)
        if len(agent.buffer["obs"]) >= MIN_TRANSITIONS:
            agent.update()
        if len(returns) % REPORT_EVERY == 0:
            recent = statistics.fmean(returns[-REPORT_EVERY:])
            print(f"episode {len(returns):5d}  mean return of the last {REPORT_EVERY}: {recent:8.2f}")
            if recent > best:
                best = recent
                agent.save(str(CKPT_DIR / "best_abr_agent.pt"))
    agent.save(str(CKPT_DIR / "final_abr_agent.pt"))
    print(f"done: {len(returns)} episodes, best ten-episode mean {best:.2f}")


def train_device(args) -> None:
    agent = new_agent(args)
    env = VecStreamingEnv(args.num_envs, max_steps=100, seed=args.seed, device=torch.device(args.device))
    rounds = max(1, args.num_steps // (args.num_envs * args.rollout_steps))
    print(f"{args.num_envs} environments on {args.device}, {rounds} rounds of {args.rollout_steps} steps, "
          f"act: {'fused kernel' if agent.fused else 'torch composition'}")
    best, seen_sum, seen_n = float("-inf"), 0.0, 0.0
    for r in range(1, rounds + 1):
        agent.collect(env, args.rollout_steps)
        m = agent.update()
        n = m["episodes_finished"] - seen_n
        if n > 0:
            mean_return = (m["episode_return_sum"] - seen_sum) / n
            seen_sum, seen_n = m["episode_return_sum"], m["episodes_finished"]
            print(f"round {r:4d}  {int(n):6d} episodes  mean return {mean_return:8.2f}  loss {m['loss']:.4f}  "
                  f"kl {m['approx_kl']:.2e}  clipped {m['clip_fraction']:.2f}")
            if mean_return > best:
                best = mean_return
                agent.save(str(CKPT_DIR / "best_abr_agent.pt"))
    agent.save(str(CKPT_DIR / "final_abr_agent.pt"))
    print(f"done: best mean return {best:.2f}")


def evaluate(args, n_episodes: int = 10) -> None:
    agent = new_agent(args)
    agent.load(args.model_path)
    returns = []
    for ep_return, info in episodes(StreamingEnv(max_steps=100), agent, None, greedy=True, seed=args.seed):
        returns.append(ep_return)
        print(f"episode {len(returns):2d}  return {ep_return:8.2f}  final VMAF {info['vmaf']:.1f}")
        if len(returns) == n_episodes:
            break
    print(f"mean return {statistics.fmean(returns):.2f}, deviation {statistics.pstdev(returns):.2f}")


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--mode", choices=["train", "eval"], default="train")
    ap.add_argument("--num-steps", type=int, default=100000, help="environment steps in total")
    ap.add_argument("--learning-rate", type=float, default=3e-4)
    ap.add_argument("--device", type=str, default="cpu")
    ap.add_argument("--model-path", type=str, default=str(CKPT_DIR / "best_abr_agent.pt"))
    ap.add_argument("--num-envs", type=int, default=1, help="environments stepped together; 1 on the cpu is the single-stream loop")
    ap.add_argument("--rollout-steps", type=int, default=128, help="steps of every environment per collect")
    ap.add_argument("--seed", type=int, default=0)
    return ap


def main() -> None:
    args = build_parser().parse_args()
    CKPT_DIR.mkdir(exist_ok=True)
    if args.mode == "eval":
        evaluate(args)
    elif args.device == "cpu" and args.num_envs == 1:
        train_host(args)
    else:
        train_device(args)


if __name__ == "__main__":
    main()
