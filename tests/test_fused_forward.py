"""fused_forward config validation (no GPU needed)."""

import pytest
import torch

from nn_distributed_training_amd.ops.stacked import resolve_fused_forward

F32, F64 = torch.float32, torch.float64


def test_fused_forward_values():
    assert resolve_fused_forward({}, F32, 1, env={}) is False
    assert resolve_fused_forward({"fused_forward": False}, F64, 0) is False
    assert resolve_fused_forward({"fused_forward": True}, F32, 1) is True
    with pytest.raises(ValueError):  # true needs the bf16 operands
        resolve_fused_forward({"fused_forward": True}, F32, 0)
    with pytest.raises(ValueError):
        resolve_fused_forward({"fused_forward": True}, F64, 0)
    for bad in ("true", 1, None):
        with pytest.raises(ValueError):
            resolve_fused_forward({"fused_forward": bad}, F32, 1)
    # NDTA_FUSED_FWD only fills an unset key, and only under bf16
    env = {"NDTA_FUSED_FWD": "1"}
    assert resolve_fused_forward({}, F32, 1, env=env) is True
    assert resolve_fused_forward({}, F32, 0, env=env) is False  # ignored
    assert resolve_fused_forward({}, F64, 0, env=env) is False
    conf = {"fused_forward": False}
    assert resolve_fused_forward(conf, F32, 1, env=env) is False
