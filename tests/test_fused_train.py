"""fused_train config validation (no GPU needed)."""

import pytest
import torch

from nn_distributed_training_amd.ops.stacked import resolve_fused_train

F32, F64 = torch.float32, torch.float64
ENV = {"NDTA_FUSED_TRAIN": "1"}


@pytest.mark.parametrize(
    "conf,dtype,prec,env,want",
    [
        ({}, F32, 1, {}, False),                      # default off
        ({"fused_train": False}, F64, 0, {}, False),
        ({"fused_train": True}, F32, 1, {}, True),
        # the env switch only fills an unset key, and only under bf16
        ({}, F32, 1, ENV, True),
        ({}, F32, 0, ENV, False),
        ({}, F64, 0, ENV, False),
        ({"fused_train": False}, F32, 1, ENV, False),
    ],
)
def test_fused_train_values(conf, dtype, prec, env, want):
    assert resolve_fused_train(conf, dtype, prec, env=env) is want


@pytest.mark.parametrize(
    "value,dtype,prec",
    [(True, F32, 0), (True, F64, 0), ("true", F32, 1), (1, F32, 1),
     (None, F32, 1)],
)
def test_fused_train_rejects(value, dtype, prec):
    with pytest.raises(ValueError):
        resolve_fused_train({"fused_train": value}, dtype, prec, env={})
