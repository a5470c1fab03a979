"""Multi-agent decentralized PPO driver.

Capability parity with the reference's
``RL/dist_rl/train_{cadmm,dsgd,dsgt}_multi.py`` (one file per algorithm
with hardcoded configs; here one driver + --alg flag and the same
defaults: 3 predators on a wheel graph, heuristic prey, obstacles).
Run: python -m nn_distributed_training_amd.rl.train_multi --alg dinno
"""

from __future__ import annotations

import argparse

import networkx as nx
import torch

from .dist_ppo import DistPPOProblem
from .envs import SimpleTagEnv
from .ppo_optimizers import build_ppo_optimizer


def default_conf(alg: str) -> dict:
    conf = {
        "timesteps_per_batch": 600,
        "max_timesteps_per_episode": 100,
        "gamma": 0.99,
        "clip": 0.2,
        "cov": 0.5,
        "max_rl_timesteps": 100_000,
        "save_freq": 10,
        "verbose": True,
        "run_id": "0",
        "output_dir": "./trained",
    }
    if alg in ("dinno", "cadmm"):
        conf.update(
            rho_init=0.3, rho_scaling=1.0, primal_iterations=5,
            primal_lr_start=1e-3, primal_lr_finish=1e-4,
            lr_decay_type="log", expected_iterations=200,
        )
    elif alg == "dsgd":
        conf.update(alpha0=1e-3, mu=1e-3)
    elif alg == "dsgt":
        conf.update(alpha_actor=1e-3, alpha_critic=1e-3)
    return conf


def build_parser():
    p = argparse.ArgumentParser()
    p.add_argument("--alg", default="dinno",
                   choices=["dinno", "cadmm", "dsgd", "dsgt"])
    p.add_argument("--predators", type=int, default=3)
    p.add_argument("--obstacles", type=int, default=2)
    p.add_argument("--max-timesteps", type=int, default=None)
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--out", default="./trained")
    p.add_argument(
        "--grad-engine", default="torch", choices=["torch", "stacked"],
        help="PPO gradients by per-node autograd (torch) or batched "
             "over all nodes on the HIP kernels (stacked; needs a GPU)",
    )
    p.add_argument(
        "--rollout-engine", default="host", choices=["host", "device"],
        help="rollouts by stepping the numpy env on the host (host) or "
             "a whole batch of episodes in one HIP kernel launch "
             "(device; needs a GPU; other action-noise stream than host)",
    )
    p.add_argument(
        "--gae-lambda", type=float, default=None,
        help="GAE(lambda) advantages with this lambda in [0, 1] "
             "(default: the Monte-Carlo estimator rtg - V, GAE's "
             "lambda = 1 corner)",
    )
    p.add_argument(
        "--critic-target", default="rtg", choices=["rtg", "lambda"],
        help="regress the critic on the rewards-to-go (rtg) or on the "
             "lambda-returns (lambda; needs --gae-lambda)",
    )
    p.add_argument(
        "--bootstrap-truncated", action="store_true",
        help="treat every episode end as the time-limit truncation it "
             "is: continue returns and advantages beyond it with the "
             "critic's value of the next observation (default: the end "
             "counts as terminal)",
    )
    return p


def conf_from_args(args) -> dict:
    conf = default_conf(args.alg)
    conf["output_dir"] = args.out
    conf["grad_engine"] = args.grad_engine
    conf["rollout_engine"] = args.rollout_engine
    conf["gae_lambda"] = args.gae_lambda
    conf["critic_target"] = args.critic_target
    conf["bootstrap_truncated"] = args.bootstrap_truncated
    return conf


def main(argv=None):
    args = build_parser().parse_args(argv)

    torch.manual_seed(args.seed)
    conf = conf_from_args(args)
    if args.max_timesteps:
        conf["max_rl_timesteps"] = args.max_timesteps

    env = SimpleTagEnv(
        num_predators=args.predators, num_obstacles=args.obstacles,
        seed=args.seed,
    )
    graph = nx.wheel_graph(args.predators)
    device = torch.device(
        "cuda" if torch.cuda.is_available() else "cpu"
    )
    pr = DistPPOProblem(graph, env, device, conf)
    opt = build_ppo_optimizer(args.alg, pr, conf)
    opt.train()
    print(f"final eval (deterministic): {pr.evaluate():.2f}")


if __name__ == "__main__":
    main()
