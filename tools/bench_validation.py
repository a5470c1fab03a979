"""Time validate_all() of the stacked engine, layered vs one launch.

Stand-alone measurement (not a test, not part of bench.py) at the paper
shapes, in fp64 and fp32. --workload mnist: 10 nodes on a cycle graph,
MNISTConvNet(3, 5, 64), V = 10,000 synthetic validation images,
val_batch_size 128, DiNNO rounds. --workload density: bench.py's online
density problem with 8 nodes, FourierNet [2, 256, 64, 64, 64, 1] scale
0.05, 200 validation scans of 20 beams x 25 samples (V = 100,000),
val_batch_size 10,000, DSGT rounds. Two comparisons on the same seeded
data and parameters:

* one validate_all() call with fused_validation off (the layered path,
  the comparison) and on (ops/hip/eval.hip, ops/hip/mlp_eval.hip);
* one evaluation period of a run with evaluate_frequency 20:
  --rounds (20) step_round calls alone against the same rounds plus one
  validate_all(), off and on. The difference over the total is the
  share of the run validation takes.

Every figure is a host clock around a window that ends in a device
synchronize (validate_all() itself ends in a copy to the host), after
--warmup untimed calls; the window is repeated --repeats times, the
variants alternating, and the median with the min-max spread is
reported. Prints one JSON line per dtype.

Run: python tools/bench_validation.py [--workload density]
         [--iters 50 --repeats 7]
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

from nn_distributed_training_amd.data.mnist import (  # noqa: E402
    SyntheticMNIST,
    split_train_set,
)
from nn_distributed_training_amd.models import MNISTConvNet  # noqa: E402
from nn_distributed_training_amd.optimizers.dinno import DiNNO  # noqa: E402
from nn_distributed_training_amd.ops.stacked import (  # noqa: E402
    DiNNOStackedDriver,
    StackedEngine,
)
from nn_distributed_training_amd.problems.dist_mnist_problem import (  # noqa: E402
    DistMNISTProblem,
)


def make_driver(args, subsets, val, device, fused):
    torch.manual_seed(0)
    opt_conf = {
        "alg_name": "dinno", "rho_init": 0.5, "rho_scaling": 1.0003,
        "outer_iterations": 2000, "primal_iterations": 2,
        "primal_optimizer": "adam", "persistant_primal_opt": False,
        "primal_lr_start": 0.005, "primal_lr_finish": 0.0005,
        "lr_decay_type": "log", "profile": False,
    }
    conf = {
        "problem_name": "bench_validation", "train_batch_size": 64,
        "val_batch_size": args.val_batch_size, "verbose_evals": False,
        "metrics": ["validation_loss", "top1_accuracy"],
        "metrics_config": {"evaluate_frequency": 20},
        "optimizer_config": opt_conf, "fused_validation": fused,
    }
    pr = DistMNISTProblem(
        nx.cycle_graph(args.nodes), MNISTConvNet(3, 5, 64),
        torch.nn.NLLLoss(), subsets, val, device, conf,
    )
    pr.stacked = StackedEngine(pr)
    driver = DiNNOStackedDriver(DiNNO(pr, device, opt_conf), pr)
    driver.prepare()
    return driver


def make_density_driver(args, device, fused):
    import numpy as np

    from nn_distributed_training_amd.data.floorplan import (
        synthetic_floorplan,
        synthetic_waypoints,
    )
    from nn_distributed_training_amd.data.lidar import (
        Lidar2D,
        OnlineTrajectoryLidarDataset,
        RandomPoseLidarDataset,
    )
    from nn_distributed_training_amd.models import FourierNet
    from nn_distributed_training_amd.optimizers.dsgt import DSGT
    from nn_distributed_training_amd.ops.stacked import DSGTStackedDriver
    from nn_distributed_training_amd.problems.dist_online_dense_problem \
        import DistOnlineDensityProblem

    np.random.seed(0)
    torch.manual_seed(0)
    img = synthetic_floorplan(nx=256, ny=256, num_walls=10,
                              border_width=24, seed=0)
    lidar = Lidar2D(img, 20, 0.2, 25, 1.0, 50, 3)
    subsets = [
        OnlineTrajectoryLidarDataset(lidar, wp, 30, 100)
        for wp in synthetic_waypoints(img, args.nodes, seed=0)
    ]
    val = RandomPoseLidarDataset(lidar, args.val)
    opt_conf = {
        "alg_name": "dsgt", "alpha": 0.001, "outer_iterations": 4000,
        "init_grads": True, "profile": False,
    }
    conf = {
        "problem_name": "bench_validation", "train_batch_size": 20000,
        "val_batch_size": args.val_batch_size, "comm_radius": 120.0,
        "dynamic_graph": True, "save_models": False, "data_seed": 0,
        "verbose_evals": False, "metrics": ["validation_loss"],
        "metrics_config": {"evaluate_frequency": 20, "tloss_decay": 0.2,
                           "mesh_only_at_end": True},
        "optimizer_config": opt_conf, "fused_validation": fused,
    }
    pr = DistOnlineDensityProblem(
        FourierNet([2, 256, 64, 64, 64, 1], scale=0.05), torch.nn.BCELoss(),
        subsets, val, device, conf,
    )
    pr.stacked = StackedEngine(pr)
    driver = DSGTStackedDriver(DSGT(pr, device, opt_conf), pr)
    driver.prepare()
    return driver


def window(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e3  # ms per call


def compare(fns, iters, warmup, repeats):
    """Alternate the variants; {name: (median, min, max)} in ms."""
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    samples = {k: [] for k in fns}
    for _ in range(repeats):
        for k, fn in fns.items():
            samples[k].append(window(fn, iters))
    return {
        k: (statistics.median(v), min(v), max(v))
        for k, v in samples.items()
    }


def bench_dtype(dtype, args):
    torch.set_default_dtype(dtype)
    dev = torch.device("cuda")
    if args.workload == "density":
        off = make_density_driver(args, dev, False)
        on = make_density_driver(args, dev, True)
    else:
        subsets = split_train_set(
            SyntheticMNIST(args.train, seed=0), args.nodes, "hetero")
        val = SyntheticMNIST(args.val, seed=1)
        off = make_driver(args, subsets, val, dev, False)
        on = make_driver(args, subsets, val, dev, True)
    e_off, e_on = off.pr.stacked, on.pr.stacked
    V = e_on._stage_val()[0].shape[0]
    assert e_on._fused_val_applicable(V, min(args.val_batch_size, V))

    # a few rounds first, so that the nodes differ; then the same
    # parameters in both engines and the same numbers from both paths
    for k in range(3):
        off.step_round(k)
    e_on.theta.copy_(e_off.theta)
    if args.workload == "density":  # regression: the losses [L] alone
        l0, l1 = e_off.validate_all(), e_on.validate_all()
        mask_diff = None
    else:
        l0, a0, c0 = e_off.validate_all()
        l1, a1, c1 = e_on.validate_all()
        mask_diff = int((c0 != c1).sum())
    loss_diff = (l0 - l1).abs().max().item()

    v = compare({"off": e_off.validate_all, "on": e_on.validate_all},
                args.iters, args.warmup, args.repeats)

    def period(driver, evaluate):
        def run():
            for k in range(args.rounds):
                driver.step_round(3 + k)
            if evaluate:
                driver.pr.stacked.validate_all()
        return run

    r = compare({"rounds_only": period(off, False),
                 "eval_off": period(off, True),
                 "eval_on": period(on, True)},
                args.iters, args.warmup, args.repeats)

    def row(x):
        return {"median_ms": round(x[0], 3), "min_ms": round(x[1], 3),
                "max_ms": round(x[2], 3)}

    def share(k):
        return round((r[k][0] - r["rounds_only"][0]) / r[k][0], 3)

    out = {
        "workload": args.workload,
        "dtype": str(dtype).replace("torch.", ""),
        "nodes": args.nodes, "V": V,
        "val_batch_size": args.val_batch_size,
        "iters": args.iters, "repeats": args.repeats,
        "max_abs_loss_diff": loss_diff, "max_loss": l0.abs().max().item(),
        "mask_rows_differing": mask_diff,
        "validate_all": {k: row(x) for k, x in v.items()},
        "validate_all_speedup": round(v["off"][0] / v["on"][0], 2),
        "rounds_per_period": args.rounds,
        "period": {k: row(x) for k, x in r.items()},
        "validation_share_off": share("eval_off"),
        "validation_share_on": share("eval_on"),
    }
    print(json.dumps(out), flush=True)
    return out


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--workload", default="mnist",
                   choices=["mnist", "density"])
    p.add_argument("--nodes", type=int, default=0,
                   help="0 = workload default (10 mnist / 8 density)")
    p.add_argument("--train", type=int, default=6000)
    p.add_argument("--val", type=int, default=0,
                   help="validation images (mnist, default 10000) or "
                        "scans of 500 rows (density, default 200)")
    p.add_argument("--val-batch-size", type=int, default=0,
                   help="0 = workload default (128 mnist / 10000 density)")
    p.add_argument("--rounds", type=int, default=20)
    p.add_argument("--iters", type=int, default=50)
    p.add_argument("--warmup", type=int, default=2)
    p.add_argument("--repeats", type=int, default=7)
    p.add_argument("--dtypes", nargs="+", default=["float64", "float32"])
    args = p.parse_args(argv)
    dens = args.workload == "density"
    args.nodes = args.nodes or (8 if dens else 10)
    args.val = args.val or (200 if dens else 10000)
    args.val_batch_size = args.val_batch_size or (10000 if dens else 128)
    if not torch.cuda.is_available():
        sys.exit("bench_validation.py measures on the GPU; none found")
    for name in args.dtypes:
        bench_dtype(getattr(torch, name), args)


if __name__ == "__main__":
    main()
