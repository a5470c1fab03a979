"""The fc2 tail on MFMA (fused_mnist.hip fc_tail), through both kernels.

From y1 on, fc_block_k and fc_fwd_split_k call one device function: the
logits, dz1 and fc2 dW are 16 x 16 MFMA tiles whose operands sweep pad
rows and columns (W2 rows C..15 and columns H..63, y1 columns H..63, dZ2
columns C..15) that have to be real zeros in LDS. The cases in
fc_tail_checks.py are the smallest that reach each of those pads, the
row tails, and LDS left dirty by an earlier launch.

Which kernel ext.fc_block runs on is decided once per process
(NDTA_FC_SPLIT), so every case runs in two child processes, one per
kernel, started once for the whole file. Each output is compared with
torch fp64 autograd on the same inputs at test_fc_split_gpu's
tolerances, and the two kernels with each other.
"""

import os
import subprocess
import sys

import pytest
import torch

from fc_tail_checks import CASES, DTYPES, SENTINEL, TWICE
from test_fc_split_gpu import LOSS_SCALE, OFF, _fp_tol, _offsets

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(
    not torch.cuda.is_available(), reason="needs MI355X"
)

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
KERNELS = {"fc_block_k": "0", "fc_fwd_split_k": "1"}
CHECKED = [c for c in CASES if c != "big"]


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """{kernel: {(case, dtype): inputs and outputs}}, read-only."""
    tmp = tmp_path_factory.mktemp("fc_tail")
    procs = {}
    for kern, split in KERNELS.items():
        env = {**os.environ, "NDTA_FC_SPLIT": split,
               "PYTHONPATH": os.pathsep.join(
                   [ROOT, os.environ.get("PYTHONPATH", "")])}
        procs[kern] = subprocess.Popen(
            [sys.executable, os.path.join(HERE, "fc_tail_checks.py"),
             str(tmp / f"{kern}.pt")],
            env=env, cwd=ROOT, stdout=subprocess.PIPE,
            stderr=subprocess.STDOUT, text=True)
    out = {}
    for kern, p in procs.items():
        log, _ = p.communicate(timeout=600)
        assert p.returncode == 0, log[-2000:]
        out[kern] = torch.load(tmp / f"{kern}.pt")
    return out


_REF = {}


def _reference(case, dname, inp):
    """torch fp64 autograd on the case's inputs, computed once."""
    if (case, dname) in _REF:
        return _REF[case, dname]
    L, M, I, H, C, _ = CASES[case]
    theta, x0, Y_all, idx, _ = inp
    theta, x0 = theta.double(), x0.double()
    _, b1_off, w2_off, b2_off, n = _offsets(I, H, C)
    ref = dict(grad=torch.zeros(L, n), dx0=torch.zeros(L * M, I),
               dz1=torch.zeros(L * M, H), loss=torch.zeros(L))
    for l in range(L):
        W1 = theta[l, :H * I].reshape(H, I).clone().requires_grad_()
        b1 = theta[l, b1_off:b1_off + H].clone().requires_grad_()
        W2 = theta[l, w2_off:w2_off + C * H].reshape(C, H) \
            .clone().requires_grad_()
        b2 = theta[l, b2_off:].clone().requires_grad_()
        xl = x0[l * M:(l + 1) * M].clone().requires_grad_()
        tgt = Y_all[l][idx[l, OFF:OFF + M]]
        z1 = xl @ W1.T + b1
        z1.retain_grad()
        z2 = torch.relu(z1) @ W2.T + b2
        loss = torch.nn.functional.nll_loss(
            torch.log_softmax(z2, dim=1), tgt)
        (loss * LOSS_SCALE).backward()
        ref["loss"][l] = loss.detach()
        ref["dz1"][l * M:(l + 1) * M] = z1.grad
        ref["dx0"][l * M:(l + 1) * M] = xl.grad * (xl.detach() > 0)
        ref["grad"][l] = torch.cat([
            W1.grad.reshape(-1), b1.grad, W2.grad.reshape(-1), b2.grad])
    _REF[case, dname] = ref
    return ref


def _close(got, want, tol, what):
    diff = (got.double() - want.double()).abs().max().item()
    print(f"{what}: max |diff| {diff:.3e}")
    torch.testing.assert_close(got.double(), want.double(), **tol,
                               msg=lambda m: f"{what}: {m}")


@requires_gpu
@pytest.mark.parametrize("dname", list(DTYPES))
@pytest.mark.parametrize("case", CHECKED)
@pytest.mark.parametrize("kern", list(KERNELS))
def test_against_fp64_autograd(runs, kern, case, dname):
    """loss, dz1, dx0, fc1 dW/db and fc2 dW/db (the grad stack is all
    four), and the row behind dz1 untouched."""
    r = runs[kern][case, dname]
    ref = _reference(case, dname, r["inp"])
    tol = _fp_tol(DTYPES[dname])
    for out in r["outs"]:
        for k in ("loss", "dz1", "dx0", "grad"):
            _close(out[k], ref[k], tol, f"{kern} {case} {dname} {k}")
        assert torch.all(out["guard"] == SENTINEL)


@requires_gpu
@pytest.mark.parametrize("dname", list(DTYPES))
@pytest.mark.parametrize("kern", list(KERNELS))
def test_large_inputs_stay_finite(runs, kern, dname):
    """The case that dirties LDS for "after_big": activations near 1e3
    are far from overflow, so every output is finite."""
    (out,) = runs[kern]["big", dname]["outs"]
    for k, v in out.items():
        assert torch.isfinite(v).all(), k
    assert torch.all(out["guard"] == SENTINEL)


@requires_gpu
@pytest.mark.parametrize("dname", list(DTYPES))
@pytest.mark.parametrize("case", CHECKED)
def test_kernels_agree(runs, case, dname):
    a = runs["fc_block_k"][case, dname]
    b = runs["fc_fwd_split_k"][case, dname]
    for x, y in zip(a["inp"][:2], b["inp"][:2]):
        assert torch.equal(x, y)  # same inputs in both processes
    tol = _fp_tol(DTYPES[dname])
    for k in ("loss", "dz1", "dx0", "grad"):
        _close(a["outs"][0][k], b["outs"][0][k], tol,
               f"{case} {dname} {k}")


@requires_gpu
@pytest.mark.parametrize("dname", list(DTYPES))
@pytest.mark.parametrize("case", TWICE)
@pytest.mark.parametrize("kern", list(KERNELS))
def test_order_of_partial_sums(runs, kern, case, dname):
    """The four logit partials are added in wave order, so what no
    atomic touches is bit-equal between two runs: dz1 always, and the
    loss where a node has one row ("rows1": its loss is one atomicAdd
    onto zero; with more rows the per-row terms meet in atomic order,
    as before, and agree at the tolerance). The fc2 slices are atomic
    sums over the row tiles."""
    L, M, I, H, C, _ = CASES[case]
    a, b = runs[kern][case, dname]["outs"]
    fc1 = H * I + H
    tol = _fp_tol(DTYPES[dname])
    assert torch.equal(a["dz1"], b["dz1"])
    assert torch.equal(a["dx0"], b["dx0"])
    if M == 1:
        assert torch.equal(a["loss"], b["loss"])
    _close(a["loss"], b["loss"], tol, f"{kern} {case} {dname} loss")
    _close(a["grad"][:, fc1:], b["grad"][:, fc1:], tol,
           f"{kern} {case} {dname} fc2 slices")
