"""activation_storage config validation (no GPU needed)."""

import pytest
import torch

from nn_distributed_training_amd.ops.stacked import (
    resolve_activation_storage as resolve,
)

F32, F64 = torch.float32, torch.float64
ENV = {"NDTA_ACT_BF16": "1"}
BF = {"activation_storage": "bf16"}


@pytest.mark.parametrize(
    "conf,dtype,prec,env,want",
    [
        ({}, F32, 1, {}, False),                         # default
        ({"activation_storage": "fp32"}, F64, 0, {}, False),
        (BF, F32, 1, {}, True),
        # the env switch only fills an unset key, and only under bf16
        ({}, F32, 1, ENV, True),
        ({}, F32, 0, ENV, False),
        ({}, F64, 0, ENV, False),
        ({"activation_storage": "fp32"}, F32, 1, ENV, False),
    ],
)
def test_values(conf, dtype, prec, env, want):
    assert resolve(conf, dtype, prec, False, False, env=env) is want


@pytest.mark.parametrize(
    "conf,dtype,prec,ffwd,ftrain,env",
    [
        (BF, F32, 0, False, False, {}),      # no bf16 operands
        (BF, F64, 0, False, False, {}),
        ({"activation_storage": "fp16"}, F32, 1, False, False, {}),
        ({"activation_storage": True}, F32, 1, False, False, {}),
        (BF, F32, 1, True, False, {}),       # fused_forward
        (BF, F32, 1, False, True, {}),       # fused_train
        ({}, F32, 1, True, False, ENV),      # the env switch, same error
        ({}, F32, 1, False, True, ENV),
    ],
)
def test_rejects(conf, dtype, prec, ffwd, ftrain, env):
    with pytest.raises(ValueError):
        resolve(conf, dtype, prec, ffwd, ftrain, env=env)
