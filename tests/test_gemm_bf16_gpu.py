"""bf16-operand linear kernels (ops/hip/gemm_bf16.hip, gemm_prec = 1)
against the fp64 product of the bf16-rounded operands, L = 2, nonzero
offsets; gemm_bf16_checks has the reference and the tolerance."""

import networkx as nx
import pytest
import torch

import gemm_bf16_checks as chk
from gemm_bf16_checks import ACT, L, SCALE, TOL, bf

pytestmark = [
    pytest.mark.gpu,
    pytest.mark.skipif(not torch.cuda.is_available(), reason="needs MI355X"),
]
DEV = torch.device("cuda")


@pytest.fixture(scope="module")
def ext():
    from nn_distributed_training_amd.ops import get_ext

    return get_ext()


@pytest.fixture(autouse=True)
def _fp32_default():
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float32)
    torch.manual_seed(9)
    yield
    torch.set_default_dtype(old)


@pytest.mark.parametrize(
    "M,I,O,act,w_off,pad",
    [
        (128, 64, 64, "relu", 4, 0),       # minimum M, full tiles, 1 stage
        (128, 64, 64, "sin_relu", 5, 0),   # full tiles, odd w_off and n:
                                           # W rows not 16-byte aligned
        (129, 8, 16, "sigmoid", 4, 0),     # minimum I/O, row tail
        (130, 72, 80, "sin_relu", 3, 2),   # ragged everywhere, K tail 8,
                                           # odd w_off and n
        (192, 256, 64, "sigmoid", 8, 0),   # 4-stage pipeline
    ],
)
def test_fwd(ext, M, I, O, act, w_off, pad):
    b_off = w_off + I * O
    theta = chk.uniform(L, b_off + O + pad, dev=DEV)
    X = chk.uniform(L * M, I, dev=DEV)
    Y = torch.full((L * M, O), 7.0, device=DEV)
    Z = torch.full_like(Y, 7.0) if act == "sin_relu" else None
    ext.linear_fwd(X, theta, Y, Z, w_off, b_off, M, I, O, ACT[act], SCALE, 1)
    W = chk.weight(theta, w_off, O, I)
    z = torch.einsum("lmi,loi->lmo", bf(X).reshape(L, M, I), bf(W))
    z = (z + theta[:, None, b_off:b_off + O].double()).reshape(L * M, O)
    if Z is not None:
        torch.testing.assert_close(Z.double(), z, **TOL)
    torch.testing.assert_close(Y.double(), chk.ACT_FWD[act](z), **TOL)


@pytest.mark.parametrize(
    "M,I,O,act,Ib",
    [
        (128, 64, 64, "relu", 0),
        (128, 64, 64, "sin_relu", 2),     # z-recompute, full-tile path
        (129, 16, 8, "sigmoid", 0),       # minimum I/O of the dX MFMA
        (130, 72, 80, "sin_relu", 0),     # ragged; K (= O) tail 16; Zb
        (130, 72, 80, "sin_relu", 2),     # z-recompute, guarded path
        (192, 256, 64, "relu", 0),        # four i-tiles
        (192, 64, 256, "relu", 0),        # K = O = 256: 4-stage pipeline
    ],
)
def test_dx(ext, M, I, O, act, Ib):
    w_off = 3
    wb_off = w_off + O * I
    bb_off = wb_off + I * max(Ib, 1)
    theta = chk.uniform(L, bb_off + I + 2, dev=DEV)
    dZ = chk.uniform(L * M, O, dev=DEV)
    Xb2 = None
    if Ib:  # the below layer's pre-activation comes from its input
        Xb2 = chk.uniform(L * M, Ib, dev=DEV)
        Wb = chk.weight(theta, wb_off, I, Ib)
        zb = torch.einsum("lmj,lij->lmi", Xb2.double().reshape(L, M, Ib),
                          Wb.double())
        zb = zb + theta[:, None, bb_off:bb_off + I].double()
        zb = zb.reshape(L * M, I)
        Zb = None
    else:
        Zb = chk.uniform(L * M, I, dev=DEV, amp=2.0)
        zb = Zb.double()
    Yb = chk.ACT_FWD[act](zb).float()
    dX = torch.full((L * M, I), 7.0, device=DEV)
    ext.linear_bwd_dx(dZ, theta, dX, Yb, Zb if act == "sin_relu" else None,
                      ACT[act], SCALE, w_off, M, I, O, Xb2, wb_off, bb_off,
                      Ib, 1)
    W = chk.weight(theta, w_off, O, I)
    ref = torch.einsum("lmo,loi->lmi", bf(dZ).reshape(L, M, O), bf(W))
    ref = ref.reshape(L * M, I) * chk.ACT_BWD[act](zb, Yb.double())
    torch.testing.assert_close(dX.double(), ref, **TOL)


@pytest.mark.parametrize(
    "M,I,O,gap",  # gap: stack elements between the weights and the bias
    [
        (256, 64, 64, 0),    # baseline
        (257, 16, 64, 0),    # M tail of 1 (a chunk of one row)
        (300, 256, 64, 0),   # four i-tiles
        (272, 48, 80, 0),    # dw_kernel_for: Mfma, not Direct; ragged I, O
        (257, 16, 64, 3),    # separate db slabs and reduce launch
    ],
)
def test_dw(ext, M, I, O, gap):
    pad_lo, pad_hi, sentinel = 5, 3, 1000.0  # |dW| <= M/16 < 1000
    X = chk.uniform(L * M, I, dev=DEV, amp=0.25)
    dZ = chk.uniform(L * M, O, dev=DEV, amp=0.25)
    w_off, b_off = pad_lo, pad_lo + I * O + gap
    end = b_off + O
    g = torch.full((L, end + pad_hi), sentinel, device=DEV)
    assert ext.dw_accumulates(M, I, O)  # the one-mode call still answers
    if ext.dw_accumulates(M, I, O, 1):
        g[:, w_off:end].zero_()
    g[:, w_off + I * O:b_off] = sentinel
    ext.linear_bwd_dw(dZ, X, g, w_off, b_off, M, I, O, 1)
    dW = torch.einsum("lmo,lmi->loi", bf(dZ).reshape(L, M, O),
                      bf(X).reshape(L, M, I))
    db = dZ.double().reshape(L, M, O).sum(dim=1)  # dZ unrounded
    ref = torch.cat([dW.reshape(L, O * I), db], dim=1)
    got = torch.cat([g[:, w_off:w_off + I * O], g[:, b_off:end]], dim=1)
    torch.testing.assert_close(got.double(), ref, **TOL)
    assert (g[:, w_off + I * O:b_off] == sentinel).all()
    assert (g[:, :w_off] == sentinel).all()
    assert (g[:, end:] == sentinel).all()


@pytest.mark.parametrize("op", ["fwd", "dx", "dw"])
def test_default_path_untouched(ext, op):
    """gemm_prec = 0 passed explicitly is the call without the argument,
    bit for bit, and a shape under the op's MFMA threshold keeps its
    kernel under gemm_prec = 1 (dX at I = 8)."""
    M, I, O = (128, 64, 64) if op == "dw" else (130, 72, 80)
    theta = chk.uniform(L, I * O + O, dev=DEV)
    A = chk.uniform(L * M, I, dev=DEV)
    G = chk.uniform(L * M, O, dev=DEV)

    def run(*prec, I=I):
        if op == "fwd":
            out = torch.zeros_like(G)
            ext.linear_fwd(A, theta, out, None, 0, I * O, M, I, O, 1, 1.0,
                           *prec)
        elif op == "dx":
            out = torch.zeros(L * M, I, device=DEV)
            ext.linear_bwd_dx(G, theta, out, None, None, 0, 1.0, 0, M, I, O,
                              None, 0, 0, 0, *prec)
        else:
            out = torch.zeros_like(theta)
            ext.linear_bwd_dw(G, A, out, 0, I * O, M, I, O, *prec)
        return out

    assert torch.equal(run(), run(0))
    if op == "dx":
        assert torch.equal(run(I=8), run(1, I=8))
        assert not torch.equal(run(), run(1))


def test_engine_flag_reaches_every_layer(monkeypatch):
    """One fwd_bwd of a tiny density problem: the C++ chains and the
    per-op python path give the same grad stack bit for bit under
    gemm_precision: bf16, and it is not the native one."""
    from nn_distributed_training_amd.models import FourierNet
    from nn_distributed_training_amd.ops.stacked import StackedEngine
    from nn_distributed_training_amd.problems.dist_dense_problem import (
        DistDensityProblem,
    )

    B, N = 256, 2
    sets = [
        torch.utils.data.TensorDataset(
            torch.rand(B, 2) * 8, torch.randint(0, 2, (B,)).float())
        for _ in range(N + 1)
    ]

    def grad(mode, py_chain):
        monkeypatch.setenv("NDTA_PY_CHAIN", py_chain)
        torch.manual_seed(3)
        conf = {
            "problem_name": "bf16", "train_batch_size": B,
            "val_batch_size": B, "verbose_evals": False, "data_seed": 3,
            "metrics": ["consensus_error"], "gemm_precision": mode,
            "metrics_config": {"evaluate_frequency": 1000},
            "optimizer_config": {"alg_name": "dsgd"},
        }
        pr = DistDensityProblem(
            nx.path_graph(N), FourierNet([2, 256, 64, 64, 1], scale=0.05),
            torch.nn.BCELoss(), sets[:N], sets[N], DEV, conf,
        )
        eng = StackedEngine(pr)
        assert eng._use_chain == (py_chain == "0")
        xb, yb = eng.next_batch()
        eng.fwd_bwd(xb, yb)
        return eng.grad.clone()

    g_chain = grad("bf16", "0")
    assert torch.equal(g_chain, grad("bf16", "1"))
    assert not torch.equal(g_chain, grad("native", "0"))
