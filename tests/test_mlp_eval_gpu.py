"""One-launch density-MLP validation and prediction (ops/hip/mlp_eval.hip,
fused_validation) against plain fp64 torch on the same inputs: per-node
sum of chunk-mean losses, and the model outputs in predict mode."""

import networkx as nx
import pytest
import torch
import torch.nn.functional as Fn

pytestmark = [
    pytest.mark.gpu,
    pytest.mark.skipif(not torch.cuda.is_available(), reason="needs MI355X"),
]
DEV = torch.device("cuda")
# TOL of tests/test_ops_gpu.py
TOL = {torch.float64: dict(rtol=1e-10, atol=1e-10),
       torch.float32: dict(rtol=2e-4, atol=2e-5)}
DTYPES = [torch.float64, torch.float32]
ACT = {"none": 0, "relu": 1, "sin_relu": 2, "sigmoid": 3, "tanh": 4,
       "logsoftmax": 5}
FLAGSHIP = ([2, 256, 64, 64, 64, 1],
            ["sin_relu", "relu", "relu", "relu", "sigmoid"], 0.05)

CASES = [
    # L, V, Bv, widths, activations, scale, loss_kind (1 BCE, 2 MSE, 3 L1)
    # minimal; one partly filled tile
    (1, 16, 16, [2, 16, 16, 1], ["sin_relu", "relu", "sigmoid"], 1.0, 1),
    # flagship chain, 8 W stages, ragged tile and chunk, shared X
    (3, 37, 16, *FLAGSHIP, 1),
    # widths no multiples of 16 or 32; chunk borders inside tiles
    (2, 70, 24, [3, 72, 40, 24, 1], ["relu", "relu", "relu", "none"], 1.0, 2),
    # no trunk; Bv > V
    (2, 33, 128, [4, 40, 1], ["tanh", "tanh"], 1.0, 3),
    # in = 1; several tiles per ticket
    (2, 130, 50, [1, 64, 64, 1], ["sigmoid", "sigmoid", "none"], 1.0, 2),
]


@pytest.fixture(scope="module")
def ext():
    from nn_distributed_training_amd.ops import get_ext

    return get_ext()


def chain(widths, acts, scale=1.0):
    """(spec [nl, 7], scales [nl], n) of a chain at an odd base offset."""
    rows, off = [], 1
    for i, o, a in zip(widths, widths[1:], acts):
        rows.append([0, off, off + o * i, i, o, ACT[a], 0])
        off += o * i + o
    scales = torch.ones(len(rows), dtype=torch.float64)
    scales[0] = scale
    return torch.tensor(rows), scales, off + 2


def reference(theta, X, spec, scales):
    """fp64 model outputs [L, V, out]."""
    outs = []
    for th in theta.double():
        x = X.double()
        for (_, w, b, i, o, a, _), s in zip(spec.tolist(), scales.tolist()):
            x = Fn.linear(x, th[w:w + o * i].reshape(o, i), th[b:b + o])
            x = [x, x.relu(), (s * x).sin().relu(), x.sigmoid(), x.tanh()][a]
        outs.append(x)
    return torch.stack(outs)


def inputs(L, V, widths, acts, scale, dtype):
    g = torch.Generator().manual_seed(5)
    spec, scales, n = chain(widths, acts, scale)
    theta = 0.1 * torch.randn(L, n, generator=g, dtype=torch.float64)
    X = torch.rand(V, widths[0], generator=g, dtype=torch.float64) * 2 - 1
    if scale != 1.0:
        X *= 128
    return spec, scales, theta.to(DEV, dtype), X.to(DEV, dtype), g


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("L,V,Bv,widths,acts,scale,kind", CASES)
def test_mlp_eval(ext, dtype, L, V, Bv, widths, acts, scale, kind):
    spec, scales, theta, X, g = inputs(L, V, widths, acts, scale, dtype)
    if kind == 1:
        y = torch.rand(V, generator=g, dtype=torch.float64).round()
    else:
        y = torch.randn(V, generator=g, dtype=torch.float64)
    y = y.to(DEV, dtype)
    assert ext.mlp_eval_fusable(spec, V, Bv, kind, dtype)

    def launch(v):
        loss = torch.full((L,), 7.0, device=DEV, dtype=dtype)
        ext.mlp_eval(spec, scales, X[:v], y[:v], theta, loss, None, v, Bv,
                     kind)
        return loss

    def check(v, loss):
        yh = reference(theta, X[:v], spec, scales)[:, :, 0]
        t = y[:v].double()
        if kind == 1:
            # neither the clamp nor fp32 saturation is what is compared
            assert 0.02 < yh.min() and yh.max() < 0.98
            p = yh.clamp(1e-12, 1 - 1e-12)
            e = -(t * p.log() + (1 - t) * (1 - p).log())
        else:
            e = (yh - t) ** 2 if kind == 2 else (yh - t).abs()
        ref = torch.stack([sum(c.mean() for c in r.split(Bv)) for r in e])
        print(f"loss {loss.tolist()} ref {ref.tolist()}")
        torch.testing.assert_close(loss.double(), ref, **TOL[dtype])

    loss = launch(V)
    check(V, loss)
    assert torch.equal(loss, launch(V))  # equal bits from launch to launch
    # the workspace was left zero: another V gives the right answer
    check(V - 5, launch(V - 5))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("L,P,widths,acts,scale", [
    (2, 37, *FLAGSHIP),
    (2, 70, [3, 72, 40, 24, 2], ["relu", "relu", "relu", "none"], 1.0),
])
def test_predict(ext, dtype, L, P, widths, acts, scale):
    spec, scales, theta, X, _ = inputs(L, P, widths, acts, scale, dtype)
    assert ext.mlp_eval_fusable(spec, P, 1, 0, dtype)
    yhat = torch.full((L, P, widths[-1]), 7.0, device=DEV, dtype=dtype)
    ext.mlp_eval(spec, scales, X, None, theta, None, yhat, P, 1, 0)
    torch.testing.assert_close(
        yhat.double(), reference(theta, X, spec, scales), **TOL[dtype])


def test_not_fusable(ext):
    f64 = torch.float64
    relu3 = ["relu", "relu", "none"]
    bad = [
        (chain([5, 16, 16, 1], relu3), 1, f64),    # first-layer in
        (chain([2, 16, 65, 1], relu3), 1, f64),    # trunk out
        (chain([2, 16, 16, 5], relu3), 0, f64),    # tail out
        (chain([2, 16, 16, 1], ["relu", "relu", "logsoftmax"]), 1, f64),
        (chain([2, 16, 16, 1], relu3), 1, torch.bfloat16),
        (chain([2, 16, 16, 2], relu3), 2, f64),    # loss on a head of 2
    ]
    for (spec, _, _), kind, dtype in bad:
        assert not ext.mlp_eval_fusable(spec, 16, 16, kind, dtype)
    assert ext.mlp_eval_fusable(chain([2, 16, 16, 2], relu3)[0], 16, 16, 0,
                                f64)
    spec, scales, n = bad[1][0]
    z = torch.zeros(16, 2, device=DEV, dtype=f64)
    with pytest.raises(RuntimeError, match="mlp_eval_fusable"):
        ext.mlp_eval(spec, scales, z, z[:, 0].contiguous(),
                     torch.zeros(1, n, device=DEV, dtype=f64),
                     torch.zeros(1, device=DEV, dtype=f64), None, 16, 16, 1)


@pytest.mark.parametrize("dtype", DTYPES)
def test_engine(dtype):
    """fused_validation: true gives validate_all()'s losses from the one
    launch (same shape, dtype, device; values within TOL), and
    predict_all() the eager modules' outputs."""
    from nn_distributed_training_amd.models import FourierNet
    from nn_distributed_training_amd.ops.stacked import StackedEngine
    from nn_distributed_training_amd.problems import dist_dense_problem

    old = torch.get_default_dtype()
    torch.set_default_dtype(dtype)
    try:
        N, V = 3, 37
        torch.manual_seed(1)
        sets = [torch.utils.data.TensorDataset(
            torch.rand(m, 2) * 8, torch.randint(0, 2, (m,)).to(dtype))
            for m in (64, 64, 64, V)]
        mesh = torch.rand(29, 2, device=DEV) * 8
        out = {}
        for fused in (False, True):
            torch.manual_seed(2)
            conf = {
                "problem_name": "fv", "train_batch_size": 16,
                "val_batch_size": 16, "verbose_evals": False,
                "data_seed": 3, "metrics": ["consensus_error"],
                "fused_validation": fused,
                "metrics_config": {"evaluate_frequency": 10**9},
                "optimizer_config": {"alg_name": "dsgd"},
            }
            pr = dist_dense_problem.DistDensityProblem(
                nx.cycle_graph(N), FourierNet([2, 256, 64, 64, 1], scale=0.05),
                torch.nn.BCELoss(), sets[:N], sets[N], DEV, conf,
            )
            eng = StackedEngine(pr)
            # distinct nodes: the problem starts them from one model
            torch.manual_seed(9)
            eng.theta += 0.05 * torch.randn_like(eng.theta)
            assert eng._fused_val_applicable(V, 16) == fused
            assert eng.predict_all_applicable(29) == fused
            out[fused] = eng.validate_all()
        yhat = eng.predict_all(mesh)
        eng.flush_to_models()
        with torch.no_grad():
            eager = torch.stack([pr.models[i](mesh) for i in pr.local_nodes])
    finally:
        torch.set_default_dtype(old)
    l0, l1 = out[False], out[True]
    assert l0.shape == l1.shape == (N,) and l0.dtype == l1.dtype == dtype
    assert l0.device == l1.device
    torch.testing.assert_close(l1, l0, **TOL[dtype])
    assert yhat.shape == eager.shape and yhat.dtype == eager.dtype
    torch.testing.assert_close(yhat, eager, **TOL[dtype])
