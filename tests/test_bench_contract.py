"""bench.py driver-contract test: flags accepted, one JSON line with the
required schema, whole-job value semantics."""

import json
import os
import subprocess
import sys

import numpy as np
import pytest

REQUIRED = {
    "metric", "value", "unit", "n_gpus", "steps", "warmup",
    "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
    "dtype", "data", "config",
}

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args):
    env = {**os.environ, "NDTA_BENCH_SUSTAIN_S": "0.5"}
    out = subprocess.run(
        [sys.executable, os.path.join(ROOT, "bench.py"), *args],
        capture_output=True, text=True, timeout=420, env=env, cwd=ROOT,
    )
    assert out.returncode == 0, out.stderr[-2000:]
    line = out.stdout.strip().splitlines()[-1]
    return json.loads(line)


def _load_dump(out_dir):
    return {f: np.load(os.path.join(out_dir, f))
            for f in sorted(os.listdir(out_dir))}


DSGD_ARGS = ["--alg", "dsgd", "--nodes", "4", "--steps", "3",
             "--warmup", "1", "--samples-per-node", "256"]


@pytest.fixture(scope="module")
def dsgd_plain_run(tmp_path_factory):
    """One plain DSGD run with its dumped outputs, shared by the tests
    below (read-only)."""
    out_dir = tmp_path_factory.mktemp("dsgd_dump")
    d = _run([*DSGD_ARGS, "--dump-outputs", str(out_dir)])
    return d, _load_dump(out_dir)


def test_bench_default_contract(tmp_path):
    d = _run(["--steps", "4", "--warmup", "1",
              "--samples-per-node", "256", "--full",
              "--dump-outputs", str(tmp_path)])
    assert REQUIRED <= set(d)
    assert d["metric"] == "comm_rounds_per_sec"
    assert d["n_gpus"] == 1
    assert d["steps"] == 4 and d["warmup"] == 1
    assert d["higher_is_better"] is True
    assert d["scaling"] == "strong"
    assert d["data"] == "synthetic"
    assert d["dtype"] == "fp64"
    assert d["value"] > 0
    # internal consistency: ms_per_step == 1e3 / rounds_per_sec
    assert abs(d["ms_per_step"] * d["value"] - 1e3) < 1e-6 * 1e3
    cfg = d["config"]
    assert cfg["nodes"] == 8 and cfg["alg"] == "dinno"
    assert "consensus_err_max" in cfg and "val_acc_max" in cfg
    assert "parallelism" in cfg
    # sustained-window evidence keys
    assert d["timed_region_s"] > 0
    assert d["sustained_rounds_per_sec"] > 0
    assert d["sustained_s"] > 0 and d["sustained_steps"] >= 1
    assert "per_step_ms_p50" in d and "per_step_ms_std" in d
    # DiNNO's round leaves parameters and duals, one row per node
    dump = _load_dump(tmp_path)
    assert set(dump) == {"theta.npy", "duals.npy"}
    for a in dump.values():
        assert a.dtype == np.float64 and a.shape == (8, 28440)
        assert np.isfinite(a).all() and np.abs(a).max() > 0


def test_bench_dsgd_config2(dsgd_plain_run):
    d, _ = dsgd_plain_run
    assert d["config"]["alg"] == "dsgd"
    assert d["config"]["nodes"] == 4


def test_bench_plain_run_is_lean(dsgd_plain_run):
    """A plain run reports the headline schema and nothing that takes
    extra stepping or an evaluation pass."""
    d, _ = dsgd_plain_run
    assert REQUIRED <= set(d)
    assert d["steps"] == 3 and d["warmup"] == 1
    assert abs(d["ms_per_step"] * d["value"] - 1e3) < 1e-6 * 1e3
    assert not [k for k in d if k.startswith("sustained_")]
    assert "timing_breakdown_ms" not in d
    assert "consensus_err_max" not in d["config"]
    assert "val_acc_max" not in d["config"]


def test_bench_dump_outputs_repeatable(tmp_path):
    """Same arguments -> the same dumped outputs, also after enough
    rounds for training to blow rounding noise up."""
    import torch

    # On the GPU the kernels' unordered fp64 atomic sums differ by
    # rounding from run to run and DiNNO/Adam training amplifies that to
    # ~1e-2 within 100 rounds; the golden CPU engine is bitwise
    # repeatable, so a few rounds do there (it runs ~16 rounds/s).
    steps = "150" if torch.cuda.is_available() else "3"
    args = ["--steps", steps, "--warmup", "2", "--samples-per-node", "256"]
    dumps = []
    for name in ("a", "b"):
        _run([*args, "--dump-outputs", str(tmp_path / name)])
        dumps.append(_load_dump(tmp_path / name))
    a, b = dumps
    assert set(a) == set(b) == {"theta.npy", "duals.npy"}
    assert sum(x.nbytes for x in a.values()) <= 64 << 20
    for f in a:
        x, y = a[f], b[f]
        assert x.dtype == np.float64 and x.shape == (8, 28440)
        assert np.isfinite(x).all() and np.abs(x).max() > 0
        # The dumped round starts from the state saved after two
        # rounds, so the two runs can differ only by the rounding of
        # three rounds' sums: relative 1e-16 per addition on weights
        # and duals of order 0.1 to 1 (4e-14 measured after 5 rounds on
        # an MI355X). Other initial weights would differ by their own size,
        # and another batch moves each weight by about the Adam step,
        # 5e-3..5e-4: 1e-9 lies orders of magnitude from both.
        assert np.abs(x - y).max() <= 1e-9
