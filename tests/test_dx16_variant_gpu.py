"""mfma_dx16_k, the single-buffered A/B variant of the MFMA dX kernel.

ext.linear_bwd_dx reads NDTA_DX_NEW once per process and no other test
sets it, so the variant kernel (NDTA_DX_NEW=0) runs here in one fresh
child process: this file, run as a script, computes the cases below and
saves every output with its sentinel guards. The cases are two of
test_linear_epilogues_gpu's: a shape with ragged m- and i-edge tiles
under a relu below layer (Yb masks), and an all-full-tile shape under
the sin_relu encode recomputed from its Ib = 2 input, in fp64 and fp32.
Each result is compared with that file's fp64 autograd reference at its
tolerances, with its rule for fp32 elements at the sin_relu kink.
"""

import os
import subprocess
import sys

import pytest
import torch

from test_linear_epilogues_gpu import (
    ACT, GUARD, KINK_MIN_F64, KINK_SHARE_MAX, KINK_SKIP, L, SCALE, TOL,
    _assert_guards, _guarded, _report, dx_case, dx_kink_stats,
)

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(
    not torch.cuda.is_available(), reason="needs MI355X"
)

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

CASES = [((150, 70, 40), "relu"), ((128, 64, 8), "sin_relu_ib2")]
DTYPES = {"fp64": torch.float64, "fp32": torch.float32}


def _child(path):
    """Runs in the NDTA_DX_NEW=0 process: {(M, I, O, variant, dtype
    name): guarded dX buffer on the CPU}."""
    from nn_distributed_training_amd.ops import get_ext

    assert os.environ.get("NDTA_DX_NEW") == "0"
    ext = get_ext()
    dev = torch.device("cuda")
    out = {}
    for (M, I, O), variant in CASES:
        for dname, dtype in DTYPES.items():
            c = dx_case(dtype, M, I, O, variant)
            buf, flat = _guarded(L * M * I, dtype)
            dX = flat.view(L * M, I)
            Xb2 = None
            if c["recompute"]:
                Xb2 = c["Xb2"].reshape(L * M, c["Ib"]).to(dev)
            theta = c["theta"].to(dev)
            ext.linear_bwd_dx(
                c["dZ"].to(dev), theta, dX, c["Yb"].to(dev), None,
                ACT[c["act"]], SCALE, c["w_off"], M, I, O, Xb2,
                c["wb_off"], c["bb_off"], c["Ib"])
            assert torch.equal(theta.cpu(), c["theta"]), \
                f"{M}x{I}x{O} {variant} {dname}: parameters changed"
            out[M, I, O, variant, dname] = buf.cpu()
    torch.save(out, path)


@pytest.fixture(scope="module")
def dx16(tmp_path_factory):
    path = tmp_path_factory.mktemp("dx16") / "dx16.pt"
    env = {**os.environ, "NDTA_DX_NEW": "0",
           "PYTHONPATH": os.pathsep.join(
               [ROOT, HERE, os.environ.get("PYTHONPATH", "")])}
    env.pop("NDTA_GEMM_BF16", None)
    r = subprocess.run(
        [sys.executable, os.path.abspath(__file__), str(path)], env=env,
        cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
        text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:]
    return torch.load(path)


@requires_gpu
@pytest.mark.parametrize("dname", list(DTYPES))
@pytest.mark.parametrize("shape,variant", CASES)
def test_dx16_fused_act_matches_autograd(dx16, shape, variant, dname):
    M, I, O = shape
    dtype = DTYPES[dname]
    c = dx_case(dtype, M, I, O, variant)
    buf = dx16[M, I, O, variant, dname]
    got = buf[GUARD:GUARD + L * M * I].view(L * M, I)
    ref = c["ref"]
    tag = f"dx16 {M}x{I}x{O} {variant} {dname}"
    if c["recompute"]:
        kmin, share = dx_kink_stats(c)
        print(f"{tag} min|sin| = {kmin:.3e} skip share = {share:.2e}")
        if dtype == torch.float64:
            assert kmin > KINK_MIN_F64
        else:
            assert share <= KINK_SHARE_MAX
            got = torch.where(c["kink"] < KINK_SKIP, ref.to(dtype), got)
    _report(tag, got, ref)
    torch.testing.assert_close(got, ref.to(dtype), **TOL[dtype])
    _assert_guards(buf, tag)


if __name__ == "__main__":
    _child(sys.argv[1])
