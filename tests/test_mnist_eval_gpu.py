"""One-launch MNIST validation (ops/hip/eval.hip, fused_validation)
against plain fp64 torch on the same inputs: per-node sum of chunk-mean
NLL and the top-1 mask. A row whose two best reference logits lie closer
than MARGIN may flip its argmax under rounding and is left out of the
mask comparison; at most 2 rows per node may be (on the CPU these inputs
give at most 1 at 1e-4 and none at 1e-10)."""

import networkx as nx
import pytest
import torch
import torch.nn.functional as Fn

pytestmark = [
    pytest.mark.gpu,
    pytest.mark.skipif(not torch.cuda.is_available(), reason="needs MI355X"),
]
DEV = torch.device("cuda")
# fp64: TOL of tests/test_ops_gpu.py; fp32: tests/test_fc_split_gpu.py's
# tolerance for the same conv -> fc1 -> fc2 -> log-softmax chain
TOL = {torch.float64: dict(rtol=1e-10, atol=1e-10),
       torch.float32: dict(rtol=1e-3, atol=1e-4)}
MARGIN = {torch.float64: 1e-10, torch.float32: 1e-4}

CASES = [
    # L, V, Bv, F, K, H, C
    (1, 16, 16, 3, 5, 64, 10),   # minimal; one partly filled tile
    (3, 37, 16, 3, 5, 64, 10),   # ragged last tile and chunk; shared X
    (2, 70, 24, 3, 5, 24, 16),   # H % 16 != 0; C = 16; chunk borders
                                 # inside tiles
    (2, 33, 33, 2, 3, 64, 10),   # guarded conv path; I = 338
    (1, 40, 128, 1, 7, 16, 3),   # K = 7; Bv > V; I = 121 odd
    (2, 130, 50, 3, 5, 40, 10),  # more tiles than one ticket round
]


@pytest.fixture(scope="module")
def ext():
    from nn_distributed_training_amd.ops import get_ext

    return get_ext()


def reference(theta, X, y, offs, F, K, H, C, Bv):
    """fp64 (loss_sum [L], correct [L, V], top-2 logit margin [L, V])."""
    cw, cb, w1, b1, w2, b2 = offs
    V = X.shape[0]
    P = (28 - K + 1) // 2
    I = F * P * P
    loss, corr, marg = [], [], []
    for th in theta.double():
        x = Fn.conv2d(X.double().reshape(V, 1, 28, 28),
                      th[cw:cw + F * K * K].reshape(F, 1, K, K),
                      th[cb:cb + F])
        x = Fn.max_pool2d(Fn.relu(x), 2).flatten(1)
        x = Fn.relu(Fn.linear(x, th[w1:w1 + H * I].reshape(H, I),
                              th[b1:b1 + H]))
        z = Fn.linear(x, th[w2:w2 + C * H].reshape(C, H), th[b2:b2 + C])
        nll = Fn.nll_loss(Fn.log_softmax(z, dim=1), y, reduction="none")
        loss.append(sum(c.mean() for c in nll.split(Bv)))
        corr.append(z.argmax(dim=1) == y)
        top = z.topk(2, dim=1).values
        marg.append(top[:, 0] - top[:, 1])
    return torch.stack(loss), torch.stack(corr), torch.stack(marg)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("L,V,Bv,F,K,H,C", CASES)
def test_mnist_eval(ext, dtype, L, V, Bv, F, K, H, C):
    g = torch.Generator().manual_seed(5)
    P = (28 - K + 1) // 2
    I = F * P * P
    sizes = [F * K * K, F, H * I, H, C * H, C]
    offs = [1 + sum(sizes[:i]) for i in range(6)]  # odd base offset
    n = 1 + sum(sizes) + 2
    theta = (0.1 * torch.randn(L, n, generator=g, dtype=torch.float64)).to(
        DEV, dtype)
    X = torch.rand(V, 784, generator=g, dtype=torch.float64).to(DEV, dtype)
    y = torch.randint(C, (V,), generator=g).to(DEV)
    assert ext.mnist_eval_fusable(F, K, H, C, 28, V, Bv, dtype)

    def launch(v):
        correct = torch.zeros(L, v, device=DEV, dtype=torch.bool)
        loss = torch.full((L,), 7.0, device=DEV, dtype=dtype)
        ext.mnist_eval(X[:v], y[:v], theta, correct, loss, *offs, F, K, H,
                       C, 28, v, Bv)
        return loss, correct

    def check(v, loss, correct):
        rl, rc, rm = reference(theta, X[:v], y[:v], offs, F, K, H, C, Bv)
        print(f"loss {loss.tolist()} ref {rl.tolist()}")
        torch.testing.assert_close(loss.double(), rl, **TOL[dtype])
        sure = rm >= MARGIN[dtype]
        assert int((~sure).sum(dim=1).max()) <= 2
        assert torch.equal(correct[sure], rc[sure])

    loss, correct = launch(V)
    check(V, loss, correct)
    again, _ = launch(V)
    assert torch.equal(loss, again)  # bit-identical from launch to launch
    # the workspace was left zero: another V gives the right answer
    check(V - 5, *launch(V - 5))


def test_not_fusable(ext):
    f64 = torch.float64
    assert not ext.mnist_eval_fusable(3, 8, 64, 10, 28, 16, 16, f64)
    assert not ext.mnist_eval_fusable(3, 5, 65, 10, 28, 16, 16, f64)
    assert not ext.mnist_eval_fusable(3, 5, 64, 17, 28, 16, 16, f64)
    assert not ext.mnist_eval_fusable(3, 5, 64, 10, 32, 16, 16, f64)
    assert not ext.mnist_eval_fusable(3, 5, 64, 10, 28, 16, 16,
                                      torch.bfloat16)
    z = torch.zeros(16, 784, device=DEV, dtype=f64)
    with pytest.raises(RuntimeError, match="mnist_eval_fusable"):
        ext.mnist_eval(z, torch.zeros(16, device=DEV, dtype=torch.long),
                       torch.zeros(1, 40000, device=DEV, dtype=f64),
                       torch.zeros(1, 16, device=DEV, dtype=torch.bool),
                       torch.zeros(1, device=DEV, dtype=f64),
                       0, 0, 0, 0, 0, 0, 3, 5, 65, 10, 28, 16, 16)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_engine(dtype):
    """fused_validation: true gives validate_all()'s triple from the one
    launch: same mask and accuracy, loss within TOL, same shapes/dtypes."""
    from nn_distributed_training_amd.data.mnist import (
        SyntheticMNIST,
        split_train_set,
    )
    from nn_distributed_training_amd.models import MNISTConvNet
    from nn_distributed_training_amd.ops.stacked import StackedEngine
    from nn_distributed_training_amd.problems.dist_mnist_problem import (
        DistMNISTProblem,
    )

    old = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        N = 3
        subsets = split_train_set(SyntheticMNIST(96, seed=0), N, "random")
        val = SyntheticMNIST(37, seed=1)
        out = {}
        for fused in (False, True):
            torch.manual_seed(2)
            conf = {
                "problem_name": "fv", "train_batch_size": 16,
                "val_batch_size": 16, "verbose_evals": False,
                "metrics": ["consensus_error"], "fused_validation": fused,
                "metrics_config": {"evaluate_frequency": 10**9},
                "optimizer_config": {"alg_name": "dsgd"},
            }
            pr = DistMNISTProblem(
                nx.cycle_graph(N), MNISTConvNet(3, 5, 64),
                torch.nn.NLLLoss(), subsets, val, DEV, conf,
            )
            eng = StackedEngine(pr)
            # distinct nodes: the problem starts them from one model
            torch.manual_seed(9)
            eng.theta +=0.05 * torch.randn_like(eng.theta)
            assert eng._fused_val_applicable(37, 16) == fused
            out[fused] = eng.validate_all()
    finally:
        torch.set_default_dtype(old)
    (l0, a0, c0), (l1, a1, c1) = out[False], out[True]
    assert torch.equal(c0, c1) and torch.equal(a0, a1)
    torch.testing.assert_close(l1, l0, **TOL[dtype])
    for u, w in zip(out[False], out[True]):
        assert u.shape == w.shape and u.dtype == w.dtype
        assert u.device == w.device
