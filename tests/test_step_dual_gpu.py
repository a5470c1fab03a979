"""The DiNNO dual ascent folded into the round's first primal step
(ext.fused_step_dual, elementwise.hip fused_step_dual_k).

The fused launch must give, bit for bit, what ext.dinno_dual_threg
followed by ext.fused_step give on the same inputs: the operations are
elementwise and in the same order, so there is no tolerance. Only the
driver-level test has one, because the backward's atomics are unordered:
it allows 10x the difference two old-path runs show between themselves.
"""

import itertools

import pytest
import torch

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(
    not torch.cuda.is_available(), reason="needs MI355X"
)

RHO, LR, B1, B2, EPS = 0.37, 0.005, 0.9, 0.999, 1e-8


@pytest.fixture(scope="module")
def ext():
    from nn_distributed_training_amd.ops import get_ext

    return get_ext()


def _csr(nbrs, dev):
    offs, idx = [0], []
    for row in nbrs:
        idx += row
        offs.append(len(idx))
    mk = lambda x: torch.tensor(x, dtype=torch.int32, device=dev)
    return mk(offs), mk(idx), mk([len(r) for r in nbrs])


def _both(ext, dtype, nbrs, n, n_remote=0, mode=0, wd=0.0, first=True,
          zero_grad=True, step_t=None, expect_fused=True):
    """Old pair and new entry on clones of one random state; returns
    (old, new) dicts after asserting bit-equality of every tensor."""
    dev = torch.device("cuda")
    L = len(nbrs)
    assert ext.step_dual_fused_for(L, 1) == expect_fused
    g = torch.Generator(device="cuda").manual_seed(1234 + 7 * L + n)
    rnd = lambda *sh: torch.randn(*sh, dtype=dtype, device=dev, generator=g)
    st = dict(theta=rnd(L, n), grad=rnd(L, n), duals=rnd(L, n),
              s=rnd(L, n), m=rnd(L, n) * 0.1, v=rnd(L, n).abs() * 0.01)
    remote = rnd(n_remote, n) if n_remote else None
    offs, idx, deg = _csr(nbrs, dev)
    step_t = step_t if step_t is not None else (1 if first else 3)
    old = {k: t.clone() for k, t in st.items()}
    new = {k: t.clone() for k, t in st.items()}
    mv = lambda d: (None, None) if mode == 2 else (d["m"], d["v"])

    ext.dinno_dual_threg(old["theta"], remote, offs, idx, old["duals"],
                         old["s"], RHO)
    ext.fused_step(old["theta"], old["grad"], old["duals"], old["s"], deg,
                   *mv(old), RHO, LR, B1, B2, EPS, wd, step_t, mode, first,
                   1, zero_grad)
    ext.fused_step_dual(new["theta"], new["grad"], remote, offs, idx, deg,
                        new["duals"], new["s"], *mv(new), RHO, LR, B1, B2,
                        EPS, wd, step_t, mode, first, 1, zero_grad)
    torch.cuda.synchronize()
    for k in st:
        assert torch.equal(old[k], new[k]), k
    assert torch.isfinite(new["theta"]).all()
    return st, new


@requires_gpu
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("first", [True, False])
def test_hazard_complete_graph(ext, dtype, first):
    """Every node reads every other node's theta: a theta store that
    overtakes another node's theta load shows here. n = 5000 is several
    blocks and no multiple of any block size."""
    L = 8
    nbrs = [[j for j in range(L) if j != i] for i in range(L)]
    st, new = _both(ext, dtype, nbrs, 5000, first=first)
    assert not torch.equal(st["theta"], new["theta"])
    assert not torch.equal(st["duals"], new["duals"])


@requires_gpu
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_path_with_isolated_node(ext, dtype):
    """Degrees 1, 2, 1, 0: the isolated node is frozen whole."""
    st, new = _both(ext, dtype, [[1], [0, 2], [1], []], 1000, first=False)
    for k in ("theta", "m", "v", "duals"):
        assert torch.equal(new[k][3], st[k][3]), k
        assert not torch.equal(new[k][:3], st[k][:3]), k
    assert (new["s"][3] == 0).all()
    assert (new["grad"] == 0).all()


@requires_gpu
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_remote_rows(ext, dtype):
    """Two received rows (table rows 3 and 4) among the neighbours, in
    an order that is not ascending."""
    _both(ext, dtype, [[3, 1], [0, 2], [4, 1, 0]], 257, n_remote=2)


@requires_gpu
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_modes_wd_zero_grad(ext, dtype):
    ring = [[2, 1], [0, 2], [1, 0]]
    for mode, wd, zg, first in itertools.product(
            (0, 1, 2), (0.0, 0.01), (True, False), (True, False)):
        st, new = _both(ext, dtype, ring, 257, mode=mode, wd=wd,
                        first=first, zero_grad=zg)
        if zg:
            assert (new["grad"] == 0).all()
        else:
            assert torch.equal(new["grad"], st["grad"])


@requires_gpu
def test_dispatch_bounds(ext):
    """Sixteen local nodes fill the fused kernel's block (64 columns x
    16 nodes = 1024 threads); seventeen are one past it, and per-tile
    gradient slabs keep the two launches too. The entry point then
    issues those two itself."""
    assert ext.step_dual_fused_for(16, 1)
    assert not ext.step_dual_fused_for(17, 1)
    assert not ext.step_dual_fused_for(4, 2)
    for L, fused in ((16, True), (17, False)):
        ring = [[(i - 1) % L, (i + 1) % L] for i in range(L)]
        _both(ext, torch.float64, ring, 300, first=False,
              expect_fused=fused)


# ------------------------------------------------------------ driver --
def _driver(N):
    import networkx as nx

    from nn_distributed_training_amd.data.mnist import (
        SyntheticMNIST,
        split_train_set,
    )
    from nn_distributed_training_amd.models import MNISTConvNet
    from nn_distributed_training_amd.optimizers.dinno import DiNNO
    from nn_distributed_training_amd.ops.stacked import (
        DiNNOStackedDriver,
        StackedEngine,
    )
    from nn_distributed_training_amd.problems.dist_mnist_problem import (
        DistMNISTProblem,
    )

    torch.manual_seed(0)
    device = torch.device("cuda", 0)
    train = SyntheticMNIST(128 * N, seed=0)
    val = SyntheticMNIST(32, seed=1)
    subsets = split_train_set(train, N, "random")
    opt_conf = {
        "alg_name": "dinno", "rho_init": 0.5, "rho_scaling": 1.0003,
        "outer_iterations": 4, "primal_iterations": 2,
        "primal_optimizer": "adam", "persistant_primal_opt": False,
        "primal_lr_start": 0.005, "primal_lr_finish": 0.001,
        "lr_decay_type": "log", "profile": False,
    }
    prob_conf = {
        "problem_name": "step_dual", "train_batch_size": 16,
        "val_batch_size": 32, "verbose_evals": False,
        "metrics": ["consensus_error"],
        "metrics_config": {"evaluate_frequency": 10**9},
        "optimizer_config": opt_conf,
    }
    pr = DistMNISTProblem(
        nx.cycle_graph(N), MNISTConvNet(3, 5, 64), torch.nn.NLLLoss(),
        subsets, val, device, prob_conf,
    )
    pr.stacked = StackedEngine(pr)
    drv = DiNNOStackedDriver(DiNNO(pr, device, opt_conf), pr)
    drv.prepare()
    # distinct models and non-zero duals, so that the ascent matters
    g = torch.Generator(device="cuda").manual_seed(5)
    pr.stacked.theta += 0.01 * torch.randn(
        pr.stacked.theta.shape, dtype=pr.stacked.theta.dtype,
        device=device, generator=g)
    drv.duals += 0.01 * torch.randn(
        drv.duals.shape, dtype=drv.duals.dtype, device=device, generator=g)
    return drv


def _old_round(drv, k):
    """The round as it was: dual ascent at its head, then forward +
    backward and the plain step per primal iteration."""
    eng = drv.eng
    ext = eng.ext
    drv.rho *= drv.opt.rho_scaling
    rbuf, _, offs, idx, deg = drv._round_plan()
    ext.dinno_dual_threg(eng.theta, rbuf, offs, idx, drv.duals, drv.s,
                         drv.rho)
    lr = float(drv.opt.primal_lr[k])
    for pi in range(drv.pits):
        _, grad_t, nparts = eng.train_step()
        assert grad_t is eng.grad and nparts == 1
        ext.fused_step(eng.theta, grad_t, drv.duals, drv.s, deg, drv.m,
                       drv.v, drv.rho, lr, B1, B2, EPS, drv.wd, pi + 1,
                       drv.mode, pi == 0, 1, True)
        eng.grad_is_zero = True


@requires_gpu
@pytest.mark.parametrize("N,fused", [(4, True), (17, False)])
def test_driver_round(N, fused):
    """One step_round against the old round from identical state, on a
    ring of N MNIST nodes at batch 16 in fp64; N = 17 is one node past
    the fused kernel, where the round keeps its two launches."""
    prev = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        out = {}
        for name in ("old_a", "old_b", "new"):
            drv = _driver(N)
            assert drv.eng.ext.step_dual_fused_for(N, 1) == fused
            if name == "new":
                drv.step_round(0)
            else:
                _old_round(drv, 0)
            torch.cuda.synchronize()
            out[name] = (drv.eng.theta.clone(), drv.duals.clone(),
                         drv.s.clone())
    finally:
        torch.set_default_dtype(prev)
    for i, what in enumerate(("theta", "duals", "s")):
        noise = (out["old_a"][i] - out["old_b"][i]).abs().max().item()
        diff = (out["new"][i] - out["old_a"][i]).abs().max().item()
        print(f"N={N} {what}: old-vs-old {noise:.3e}  new-vs-old {diff:.3e}")
        assert diff <= 10 * noise, what
    # the ascent itself is before any atomics: exact
    assert torch.equal(out["new"][1], out["old_a"][1])
    assert torch.equal(out["new"][2], out["old_a"][2])
