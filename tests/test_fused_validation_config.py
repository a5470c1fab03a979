"""The fused_validation problem-config key (ops/stacked.py)."""

import pytest

from nn_distributed_training_amd.ops.stacked import resolve_fused_validation


def test_resolve_fused_validation():
    assert resolve_fused_validation({}, env={}) is False
    assert resolve_fused_validation({"fused_validation": True}, env={})
    assert not resolve_fused_validation({"fused_validation": False}, env={})
    # the environment switch counts only where the key is unset
    on = {"NDTA_FUSED_VAL": "1"}
    assert resolve_fused_validation({}, env=on) is True
    assert resolve_fused_validation({}, env={"NDTA_FUSED_VAL": "0"}) is False
    assert not resolve_fused_validation({"fused_validation": False}, env=on)
    with pytest.raises(ValueError, match="fused_validation"):
        resolve_fused_validation({"fused_validation": "yes"}, env={})
