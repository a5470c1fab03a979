"""The merged fc1-dW + conv-backward launch (ext.dw_conv_bwd_idx) against
the two entry points it replaces on the index-sourced path, and the
engine's single-call fwd_bwd against the layered kernel chain."""

import networkx as nx
import pytest
import torch

from test_ops_gpu import TOL

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(
    not torch.cuda.is_available(), reason="needs MI355X"
)

SENTINEL = 12345.5


@pytest.fixture(scope="module")
def ext():
    from nn_distributed_training_amd.ops import get_ext

    return get_ext()


@requires_gpu
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("L,B,F,K,IMG,H", [
    (2, 64, 3, 5, 28, 64),  # the MNIST shape
    (3, 5, 2, 3, 8, 48),    # B < 32 chunks, I = 18 is no multiple of 16
])
def test_merged_bwd_matches_separate(ext, dtype, L, B, F, K, IMG, H):
    torch.manual_seed(9)
    dev = torch.device("cuda")
    P = (IMG - (K - 1)) // 2
    I = F * P * P
    cw_off, cb_off = 0, F * K * K
    w1_off = cb_off + F
    b1_off = w1_off + H * I
    rest = b1_off + H            # stands for the fc2 slice
    n = rest + 50
    maxlen, S, off = B + 7, 2 * B + 3, 2

    dz1 = torch.randn(L * B, H, dtype=dtype, device=dev)
    x0 = torch.relu(torch.randn(L * B, I, dtype=dtype, device=dev))
    dY = torch.randn(L * B, I, dtype=dtype, device=dev)
    dY = dY * (torch.rand_like(dY) > 0.3)  # relu-masked grads have zeros
    pidx = torch.randint(0, 4, (L * B, I), device=dev).to(torch.uint8)
    X_all = torch.randn(L, maxlen, IMG * IMG, dtype=dtype, device=dev)
    src = torch.randint(0, maxlen, (L, S), device=dev)

    def fresh():
        g = torch.full((L, n), SENTINEL, dtype=dtype, device=dev)
        g[:, cw_off:w1_off] = 0  # the conv slice accumulates atomically
        return g

    ref = fresh()
    ext.linear_bwd_dw(dz1, x0, ref, w1_off, b1_off, B, I, H)
    ext.conv_pool_bwd_idx(dY, pidx, X_all, src, S, off, ref, cw_off,
                          cb_off, B, F, K, IMG)
    out = fresh()
    ext.dw_conv_bwd_idx(dz1, x0, dY, pidx, X_all, src, S, off, out,
                        w1_off, b1_off, B, I, H, cw_off, cb_off, F, K,
                        IMG)

    # fc1 dW/db: a store path with an unchanged summation order
    assert torch.equal(out[:, w1_off:rest], ref[:, w1_off:rest])
    assert not (ref[:, w1_off:rest] == SENTINEL).any()
    # conv dW/db: atomics, order varies
    torch.testing.assert_close(out[:, cw_off:w1_off],
                               ref[:, cw_off:w1_off], **TOL[dtype])
    assert ref[:, cw_off:w1_off].abs().max() > 0
    # everything else is untouched
    assert (out[:, rest:] == SENTINEL).all()


@requires_gpu
def test_engine_single_call_matches_layered(monkeypatch):
    """StackedEngine.fwd_bwd through ext.mnist_fwd_bwd == the layered
    chain (NDTA_FC_BLOCK=0) on a 2-node, batch-16 MNIST problem."""
    from nn_distributed_training_amd.data.mnist import (
        SyntheticMNIST,
        split_train_set,
    )
    from nn_distributed_training_amd.models import MNISTConvNet
    from nn_distributed_training_amd.ops.stacked import StackedEngine
    from nn_distributed_training_amd.problems.dist_mnist_problem import (
        DistMNISTProblem,
    )

    torch.set_default_dtype(torch.float64)
    nodes, batch = 2, 16
    conf = {
        "problem_name": "merged", "train_batch_size": batch,
        "val_batch_size": 16, "data_seed": 3, "verbose_evals": False,
        "metrics": ["consensus_error"],
        "metrics_config": {"evaluate_frequency": 1000},
        "optimizer_config": {
            "alg_name": "dsgd", "outer_iterations": 1, "alpha0": 0.004,
            "mu": 0.001, "profile": False,
        },
    }

    def run(fc_block):
        monkeypatch.setenv("NDTA_FC_BLOCK", "1" if fc_block else "0")
        torch.manual_seed(11)
        train = SyntheticMNIST(batch * nodes, seed=0)  # one batch/node
        val = SyntheticMNIST(16, seed=1)
        pr = DistMNISTProblem(
            nx.cycle_graph(nodes), MNISTConvNet(3, 5, 64),
            torch.nn.NLLLoss(), split_train_set(train, nodes, "random"),
            val, torch.device("cuda"), conf,
        )
        eng = pr.stacked = StackedEngine(pr)
        assert eng.fc_block_applicable() == fc_block
        xb, yb = eng.next_batch()
        loss = eng.fwd_bwd(xb, yb, want_loss=True)
        return eng.grad.clone(), loss.clone()

    g_new, loss_new = run(True)
    g_ref, loss_ref = run(False)
    assert g_ref.abs().max() > 0
    torch.testing.assert_close(g_new, g_ref, **TOL[torch.float64])
    torch.testing.assert_close(loss_new, loss_ref, **TOL[torch.float64])
