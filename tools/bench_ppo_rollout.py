"""Time the PPO tree's rollout, host env stepping vs the rollout kernel.

Stand-alone measurement (not a test, not part of bench.py) at the RL
tree's default shape: 3 nodes on a wheel graph, timesteps_per_batch 600
in episodes of 100, hidden=(64, 64, 64), in fp32 and fp64. Two
comparisons:

* one rollout() -
  "host":   DistPPOProblem.rollout() stepping the numpy env, every
            node's actor module once per step;
  "device": rollout_engine "device": resets and noise drawn, one
            ext.ppo_rollout launch, advantages from the stacked engine;
* one whole DiNNO round, rollout() + step_round() with grad_engine
  "stacked", under the two rollout engines.

With --gae-lambda LAM a third comparison times one device rollout()
under the default Monte-Carlo advantages ("mc": the eager torch chain)
against GAE(LAM) advantages ("gae": one ext.ppo_gae launch), the two
alternating like the others; the first two comparisons stay on the
default estimator.

With --kernels the two kernels are timed on their own instead, launch
by launch on fixed inputs: ext.ppo_rollout without ("off") and with
("on") the last_obs output, and ext.ppo_gae without and with v_last.
--off-only times the off launches alone: what a build from before
these arguments existed can run, for a comparison against it (run the
two trees' copies of this tool in turn, several times over).

Every figure is a host clock around a window of calls that ends in a
device synchronize, after untimed warm-up calls; the window is repeated
--repeats times, the two variants alternating, and the median with the
min-max spread is reported. A host rollout is three orders of magnitude
above the clock's resolution, so its window is --host-iters calls; the
device window is --iters calls. Prints one JSON line per dtype.

Run: python tools/bench_ppo_rollout.py [--iters 50 --repeats 5]
"""

from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import networkx as nx
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from nn_distributed_training_amd.rl.dist_ppo import DistPPOProblem  # noqa: E402
from nn_distributed_training_amd.rl.envs import SimpleTagEnv  # noqa: E402
from nn_distributed_training_amd.rl.ppo_optimizers import DiNNOPPO  # noqa: E402


def make_optimizer(args, rollout_engine, device, seed=0, gae_lambda=None):
    torch.manual_seed(seed)
    env = SimpleTagEnv(num_predators=args.nodes, num_obstacles=2,
                       seed=seed)
    conf = {"hidden": tuple(args.hidden), "verbose": False,
            "timesteps_per_batch": args.samples,
            "max_timesteps_per_episode": args.episode,
            "rollout_engine": rollout_engine,
            "grad_engine": "stacked", "gae_lambda": gae_lambda,
            "primal_iterations": args.primal_iterations,
            "rho_init": 0.3, "primal_lr_start": 1e-4,
            "primal_lr_finish": 1e-4, "lr_decay_type": "constant"}
    pr = DistPPOProblem(nx.wheel_graph(args.nodes), env, device, conf)
    return DiNNOPPO(pr, conf)


def window(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e6  # us per call


def compare(fns, iters, warmup, repeats):
    """Alternate the variants; {name: (median, min, max)} in us."""
    for k, fn in fns.items():
        for _ in range(warmup[k]):
            fn()
    samples = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            samples[k].append(window(fn, iters[k]))
    return {
        k: (statistics.median(v), min(v), max(v))
        for k, v in samples.items()
    }


def bench_dtype(dtype, args):
    torch.set_default_dtype(dtype)
    dev = torch.device("cuda")
    o_h = make_optimizer(args, "host", dev)
    o_d = make_optimizer(args, "device", dev)
    iters = {"host": args.host_iters, "device": args.iters}
    warmup = {"host": 1, "device": args.warmup}

    def round_of(opt):
        def fn():
            opt.pr.rollout()
            opt.step_round(0)
        return fn

    ro = compare({"host": o_h.pr.rollout, "device": o_d.pr.rollout},
                 iters, warmup, args.repeats)
    rd = compare({"host": round_of(o_h), "device": round_of(o_d)},
                 iters, warmup, args.repeats)

    def row(x):
        return {"median_us": round(x[0], 1), "min_us": round(x[1], 1),
                "max_us": round(x[2], 1)}

    out = {
        "dtype": str(dtype).replace("torch.", ""),
        "nodes": args.nodes, "timesteps_per_batch": args.samples,
        "episode": args.episode, "hidden": list(args.hidden),
        "primal_iterations": args.primal_iterations,
        "iters": iters, "repeats": args.repeats,
        "weights_in_lds": os.environ.get("NDTA_ROLLOUT_WLDS", "auto"),
        "rollout": {k: row(x) for k, x in ro.items()},
        "rollout_speedup": round(ro["host"][0] / ro["device"][0], 1),
        "dinno_round": {k: row(x) for k, x in rd.items()},
        "dinno_round_speedup": round(
            rd["host"][0] / rd["device"][0], 1),
    }
    if args.gae_lambda is not None:
        o_g = make_optimizer(args, "device", dev,
                             gae_lambda=args.gae_lambda)
        rg = compare({"mc": o_d.pr.rollout, "gae": o_g.pr.rollout},
                     {"mc": args.iters, "gae": args.iters},
                     {"mc": args.warmup, "gae": args.warmup},
                     args.repeats)
        out["gae_lambda"] = args.gae_lambda
        out["rollout_device_estimator"] = {
            k: row(x) for k, x in rg.items()}
    print(json.dumps(out), flush=True)
    return out


def bench_kernels(dtype, args):
    """ext.ppo_rollout and ext.ppo_gae alone, with and without the
    bootstrap's output / input, on one batch's fixed inputs."""
    from nn_distributed_training_amd.ops import get_ext

    torch.set_default_dtype(dtype)
    dev = torch.device("cuda")
    pr = make_optimizer(args, "device", dev).pr
    dr = pr.device_rollout
    M, ep_len, E = dr.shape()
    N = pr.N
    theta = pr._theta_stack()
    eps = dr.draw_noise(E, ep_len)
    resets = torch.as_tensor(
        dr.draw_resets(E), dtype=torch.float64).to(dev).contiguous()
    out = dr.run(theta, resets.cpu().numpy(), eps)
    conf = pr.conf
    ext = get_ext()
    names = ["off"] if args.off_only else ["off", "on"]

    def rollout_fn(name):
        tail = (out["last_obs"],) if name == "on" else ()

        def fn():
            ext.ppo_rollout(
                theta, *dr._plan, resets, dr._obst, eps, out["obs"],
                out["acts"], out["logp"], out["rews"], out["rtgs"],
                out["ep_rew"], M, ep_len, float(conf["cov"]),
                float(conf["gamma"]), dr._envp, *tail)
        return fn

    v = torch.randn(N * M, device=dev, dtype=dtype)
    v_last = torch.randn(N * E, device=dev, dtype=dtype)
    adv, ret = torch.empty_like(v), torch.empty_like(v)
    lam = 0.95 if args.gae_lambda is None else args.gae_lambda

    def gae_fn(name):
        tail = (v_last,) if name == "on" else ()

        def fn():
            ext.ppo_gae(v, out["rews"], 0, adv, ret, M, ep_len,
                        float(conf["gamma"]), lam, *tail)
        return fn

    iters = {k: args.kernel_iters for k in names}
    warmup = {k: args.warmup for k in names}
    ro = compare({k: rollout_fn(k) for k in names}, iters, warmup,
                 args.repeats)
    ga = compare({k: gae_fn(k) for k in names}, iters, warmup,
                 args.repeats)

    def row(x):
        return {"median_us": round(x[0], 2), "min_us": round(x[1], 2),
                "max_us": round(x[2], 2)}

    res = {
        "dtype": str(dtype).replace("torch.", ""), "nodes": N,
        "timesteps_per_batch": M, "episode": ep_len,
        "hidden": list(args.hidden), "iters": args.kernel_iters,
        "repeats": args.repeats, "gae_lambda": lam,
        "ppo_rollout_launch": {k: row(x) for k, x in ro.items()},
        "ppo_gae_launch": {k: row(x) for k, x in ga.items()},
    }
    print(json.dumps(res), flush=True)
    return res


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--nodes", type=int, default=3)
    p.add_argument("--samples", type=int, default=600)
    p.add_argument("--episode", type=int, default=100)
    p.add_argument("--hidden", type=int, nargs="+", default=[64, 64, 64])
    p.add_argument("--primal-iterations", type=int, default=5)
    p.add_argument("--iters", type=int, default=50)
    p.add_argument("--host-iters", type=int, default=1)
    p.add_argument("--warmup", type=int, default=5)
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--dtypes", nargs="+", default=["float32", "float64"])
    p.add_argument("--gae-lambda", type=float, default=None,
                   help="also time the device rollout() with GAE(lambda) "
                        "advantages against the default estimator")
    p.add_argument("--kernels", action="store_true",
                   help="time ext.ppo_rollout with/without last_obs and "
                        "ext.ppo_gae with/without v_last instead")
    p.add_argument("--kernel-iters", type=int, default=2000)
    p.add_argument("--off-only", action="store_true",
                   help="with --kernels: only the launches without the "
                        "new arguments (all an older build can run)")
    args = p.parse_args(argv)
    if not torch.cuda.is_available():
        sys.exit("bench_ppo_rollout.py measures on the GPU; none found")
    for name in args.dtypes:
        if args.kernels:
            bench_kernels(getattr(torch, name), args)
        else:
            bench_dtype(getattr(torch, name), args)


if __name__ == "__main__":
    main()
