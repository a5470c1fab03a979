"""CPU tests of ``grad_engine: "fused"``: the switch's errors without a
GPU and the ``train_multi`` command line."""

import pytest

from nn_distributed_training_amd.rl import train_multi
from nn_distributed_training_amd.rl.ppo_optimizers import (
    build_ppo_optimizer,
)
from test_ppo_stacked import _cpu_problem


def test_fused_on_cpu_fails_loudly():
    pr, conf = _cpu_problem()
    with pytest.raises(ValueError, match="grad_engine"):
        build_ppo_optimizer("dinno", pr, {**conf, "grad_engine": "fused"})
    assert pr.value_engine is None


def test_train_multi_accepts_grad_engine_fused():
    args = train_multi.build_parser().parse_args(["--grad-engine", "fused"])
    assert args.grad_engine == "fused"
