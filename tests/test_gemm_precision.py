"""gemm_precision config validation (no GPU needed)."""

import pytest
import torch

from nn_distributed_training_amd.ops.stacked import resolve_gemm_precision

F32, F64 = torch.float32, torch.float64


def test_gemm_precision_values():
    assert resolve_gemm_precision({}, F32, env={}) == 0
    assert resolve_gemm_precision({"gemm_precision": "native"}, F64) == 0
    assert resolve_gemm_precision({"gemm_precision": "bf16"}, F32) == 1
    with pytest.raises(ValueError):
        resolve_gemm_precision({"gemm_precision": "bf16"}, F64)
    with pytest.raises(ValueError):
        resolve_gemm_precision({"gemm_precision": "fp8"}, F32)
    # NDTA_GEMM_BF16 only fills an unset key, and only for fp32
    env = {"NDTA_GEMM_BF16": "1"}
    assert resolve_gemm_precision({}, F32, env=env) == 1
    assert resolve_gemm_precision({}, F64, env=env) == 0  # ignored
    conf = {"gemm_precision": "native"}
    assert resolve_gemm_precision(conf, F32, env=env) == 0
