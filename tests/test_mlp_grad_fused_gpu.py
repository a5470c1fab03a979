"""One-launch gradient kernel (ops/hip/mlp_grad_fused.hip) against a plain
fp64 backward that starts from the activations ext.mlp_fwd_fused stashes
for the same spec, theta and X: the gradient kernel calls that kernel's
forward phases, so relu-mask flips and one-ulp bf16 flips of the forward
stay out of the comparison. Trunk contractions take bf16-rounded operands
(dZ, the activation below, W), lift and tail are unrounded, every db is
the column sum of the unrounded dZ.

loss_scale = M makes the per-row weight of the mean losses 1, so gradient
entries are O(1) (up to 7e2 at the flagship chain).

Tolerance. The layered bf16 path (fwd_chain + bwd_chain, gemm_prec = 1)
against this reference at the flagship case (M = 128) misses
gemm_bf16_checks.TOL: largest error 8.206e-2, 915 times the TOL bound
(its own forward differs from the stashes in the lift's and the tail's
bits, so mask flips are in that figure). As the layered path does not
pass TOL, the bound on the gradient is TOL's rtol with atol = twice that
error, 1.641e-1. The loss keeps TOL. Measured for the fused kernel:
4.3e-5 at M = 128 (0.02 of the TOL bound, all three chains), 7.1e-3 at
M = 321 (452 of 51202 entries over the TOL bound, the same entries and
figure at max_blocks 0, 1 and 3: a bf16 rounding of one fp32 dZ entry
that the fp64 reference rounds the other way, not the work split).
"""

import networkx as nx
import pytest
import torch

import gemm_bf16_checks as chk
from gemm_bf16_checks import L, SCALE, TOL, bf

pytestmark = [
    pytest.mark.gpu,
    pytest.mark.skipif(not torch.cuda.is_available(), reason="needs MI355X"),
]
DEV = torch.device("cuda")
ACT = {**chk.ACT, "tanh": 4}
F32 = torch.float32

FLAGSHIP = ([2, 256, 64, 64, 64, 1],
            ["sin_relu", "relu", "relu", "relu", "sigmoid"])
RAGGED = ([3, 72, 40, 24, 2], ["sin_relu", "relu", "none", "tanh"])
BCE, MSE, L1 = 1, 2, 3
GRAD_TOL = dict(rtol=TOL["rtol"], atol=2 * 8.206e-2)


@pytest.fixture(scope="module")
def ext():
    from nn_distributed_training_amd.ops import get_ext

    return get_ext()


@pytest.fixture(autouse=True)
def _fp32_default():
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float32)
    yield
    torch.set_default_dtype(old)


def make_spec(widths, acts, w_off=0):
    rows, off = [], w_off
    for i, o, a in zip(widths, widths[1:], acts):
        rows.append([0, off, off + i * o, i, o, ACT[a], 0])
        off += i * o + o
    scales = torch.full((len(rows),), SCALE, dtype=torch.float64)
    return torch.tensor(rows, dtype=torch.long), scales, off


def make_case(chain, kind, M, w_off=0, pad=0):
    widths, acts = chain
    spec, scales, n = make_spec(widths, acts, w_off)
    g = torch.Generator().manual_seed(11)
    theta = (torch.rand(L, n + pad, generator=g) - 0.5).to(DEV)
    X = (torch.rand(L * M, widths[0], generator=g) - 0.5).to(DEV)
    Y = torch.rand(L * M, widths[-1], generator=g)
    Y = ((Y > 0.5).float() if kind == BCE else Y).to(DEV)
    return spec, scales, theta, X, Y


def stashes(ext, chain, spec, scales, theta, X, M):
    outs = [torch.empty(L * M, o, device=DEV) for o in chain[0][1:]]
    ext.mlp_fwd_fused(spec, scales, X, theta, outs, M)
    return outs


def reference(chain, spec, theta, X, Y, outs, kind, loss_scale, M):
    """fp64 loss [L] and gradient [L, n] from the stashed activations."""
    acts, nl = chain[1], len(chain[1])
    lay = spec[:, 1:5].tolist()
    outs = [o.double().reshape(L, M, -1) for o in outs]
    Xd = X.double().reshape(L, M, -1)
    yh, t, w = outs[-1], Y.double().reshape(L, M, -1), loss_scale / M
    if kind == BCE:
        lp = torch.log(yh.clamp_min(1e-12))
        lq = torch.log((1 - yh).clamp_min(1e-12))
        loss, dz = -(t * lp + (1 - t) * lq), (yh - t) * w
    else:
        d = yh - t
        loss = d * d if kind == MSE else d.abs()
        dy = 2 * d * w if kind == MSE else torch.sign(d) * w
        dz = dy * {"none": 1, "sigmoid": yh * (1 - yh),
                   "tanh": 1 - yh * yh}[acts[-1]]
    loss = loss.sum((1, 2)) / M
    grad = torch.zeros(L, theta.shape[1], dtype=torch.float64, device=DEV)
    for li in reversed(range(nl)):
        w_off, b_off, i, o = lay[li]
        W = chk.weight(theta, w_off, o, i).double()
        below = Xd if li == 0 else outs[li - 1]
        trunk = 0 < li < nl - 1
        dzc, A, Wc = (bf(dz), bf(below), bf(W)) if trunk else (dz, below, W)
        dW = torch.einsum("lmo,lmi->loi", dzc, A)
        grad[:, w_off:w_off + o * i] = dW.reshape(L, -1)
        grad[:, b_off:b_off + o] = dz.sum(1)
        if li == 0:
            break
        dx = torch.einsum("lmo,loi->lmi", dzc, Wc)
        if acts[li - 1] == "relu":
            dz = dx * (below > 0)
        elif acts[li - 1] == "sin_relu":  # the lift: z from X in fp64
            w0, b0, i0, o0 = lay[0]
            z = torch.einsum("lmi,loi->lmo", Xd,
                             chk.weight(theta, w0, o0, i0).double())
            z = z + theta[:, None, b0:b0 + o0].double()
            dz = dx * chk.ACT_BWD["sin_relu"](z, below)
        else:
            dz = dx
    return loss, grad


def run_fused(ext, spec, scales, theta, X, Y, kind, M, max_blocks):
    """Two launches into 7.0-filled buffers; they must agree bitwise."""
    res = []
    for _ in range(2):
        grad = torch.full_like(theta, 7.0)
        loss = torch.full((L,), 7.0, device=DEV)
        ext.mlp_grads_fused(spec, scales, X, Y, theta, grad, loss, kind,
                            float(M), M, max_blocks)
        res.append((grad, loss))
    assert torch.equal(res[0][0], res[1][0])
    assert torch.equal(res[0][1], res[1][1])
    return res[0]


@pytest.mark.parametrize(
    "chain,kind,M,max_blocks",
    [
        (FLAGSHIP, BCE, 128, 0),  # full tiles, 4 k-steps of 64, flagship LDS
        (RAGGED, MSE, 130, 0),    # row tail, ragged widths, K tails, 2-wide
        (RAGGED, L1, 130, 0),     # head, a trunk layer without activation
        (FLAGSHIP, BCE, 321, 1),  # one block, 6 tiles of both nodes:
                                  # flush at the node boundary, 1-row tile
        (FLAGSHIP, BCE, 321, 3),  # a node's tiles split over blocks: slab
                                  # sum in rank order, ticket
    ],
)
def test_grads(ext, chain, kind, M, max_blocks):
    spec, scales, theta, X, Y = make_case(chain, kind, M)
    assert ext.mlp_grads_fusable(spec, M, 1, F32, kind)
    outs = stashes(ext, chain, spec, scales, theta, X, M)
    loss_ref, grad_ref = reference(chain, spec, theta, X, Y, outs, kind,
                                   float(M), M)
    grad, loss = run_fused(ext, spec, scales, theta, X, Y, kind, M,
                           max_blocks)
    print("max |grad - ref|", (grad.double() - grad_ref).abs().max().item(),
          "max |ref|", grad_ref.abs().max().item())
    torch.testing.assert_close(loss.double(), loss_ref, **TOL)
    torch.testing.assert_close(grad.double(), grad_ref, **GRAD_TOL)


def test_unfusable_stack(ext):
    """Slices that do not tile the row (odd w_off, n padded by 1, as
    test_mlp_fused_gpu's ragged chain has them) are refused."""
    M = 130
    for w_off, pad in [(3, 1), (0, 1)]:
        spec, scales, theta, X, Y = make_case(RAGGED, MSE, M, w_off, pad)
        with pytest.raises(RuntimeError, match="mlp_grads_fusable"):
            ext.mlp_grads_fused(spec, scales, X, Y, theta,
                                torch.empty_like(theta), None, MSE, 1.0, M)


def test_dispatch(ext):
    M = 128
    spec = make_spec(*FLAGSHIP)[0]
    assert not ext.mlp_grads_fusable(spec, M, 0, F32, BCE)  # native operands
    refused = [
        (FLAGSHIP, 64),                                        # M < 128
        (([2, 256, 64, 64, 1],
          ["sin_relu", "sigmoid", "relu", "sigmoid"]), M),     # trunk act
        (([2, 64, 16], ["relu", "none"]), M),                  # no tail
        (([2, 256, 128, 1], ["relu", "relu", "sigmoid"]), M),  # wide trunk
    ]
    for chain, m in refused:
        spec, scales, theta, X, Y = make_case(chain, MSE, m)
        assert not ext.mlp_grads_fusable(spec, m, 1, F32, MSE)
        with pytest.raises(RuntimeError):
            ext.mlp_grads_fused(spec, scales, X, Y, theta,
                                torch.empty_like(theta), None, MSE, 1.0, m)


def test_engine(ext, monkeypatch):
    """fused_train: true turns a training step into one mlp_grads_fused
    call; false keeps fwd_chain + bwd_chain."""
    from nn_distributed_training_amd.models import FourierNet
    from nn_distributed_training_amd.ops.stacked import StackedEngine
    from nn_distributed_training_amd.problems.dist_dense_problem import (
        DistDensityProblem,
    )

    B, N = 256, 2
    torch.manual_seed(11)
    sets = [
        torch.utils.data.TensorDataset(
            torch.rand(B, 2) * 8, torch.randint(0, 2, (B,)).float())
        for _ in range(N + 1)
    ]
    calls = {"mlp_grads_fused": 0, "fwd_chain": 0, "bwd_chain": 0}
    real = {k: getattr(ext, k) for k in calls}

    def counted(name):
        def f(*a):
            calls[name] += 1
            return real[name](*a)
        return f

    for name in calls:
        monkeypatch.setattr(ext, name, counted(name))
    for fused in (True, False):
        torch.manual_seed(3)
        conf = {
            "problem_name": "fused", "train_batch_size": B,
            "val_batch_size": B, "verbose_evals": False, "data_seed": 3,
            "metrics": ["consensus_error"], "gemm_precision": "bf16",
            "fused_train": fused,
            "metrics_config": {"evaluate_frequency": 1000},
            "optimizer_config": {"alg_name": "dsgd"},
        }
        pr = DistDensityProblem(
            nx.path_graph(N),
            FourierNet([2, 256, 64, 64, 1], scale=0.05),
            torch.nn.BCELoss(), sets[:N], sets[N], DEV, conf,
        )
        eng = StackedEngine(pr)
        for k in calls:
            calls[k] = 0
        lb, grad, nparts = eng.train_step(want_loss=True)
        assert nparts == 1 and torch.isfinite(lb).all()
        if not fused:
            assert calls == {"mlp_grads_fused": 0, "fwd_chain": 1,
                             "bwd_chain": 1}
            continue
        assert calls == {"mlp_grads_fused": 1, "fwd_chain": 0,
                         "bwd_chain": 0}
        direct = torch.full_like(eng.grad, 7.0)
        real["mlp_grads_fused"](
            *eng._chain_meta(), eng._bufs["xb"], eng._bufs["yb"],
            eng.theta, direct, None, BCE, 1.0, B)
        assert torch.equal(grad, direct)
