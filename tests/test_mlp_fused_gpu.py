"""Whole-MLP forward kernel (ops/hip/mlp_fused.hip) layer by layer
against fp64: each layer's stash is checked against the fp64 result
computed from the kernel's OWN stash of the layer below (X for layer 0),
so a one-ulp bf16 rounding flip of an intermediate stays out of the
comparison while, by induction from X, every layer is pinned. Trunk
layers contract bf16-rounded operands (native fp32 misses that by about
2^-9 relative), lift and tail are unrounded. gemm_bf16_checks derives
the tolerance for K <= 300; here K <= 256."""

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
ACT_FWD = {**chk.ACT_FWD, "tanh": torch.tanh, "none": lambda z: z}

FLAGSHIP = ([2, 256, 64, 64, 64, 1],
            ["sin_relu", "relu", "relu", "sigmoid", "sigmoid"], 4, 0)
RAGGED = ([3, 72, 40, 24, 2], ["sin_relu", "tanh", "relu", "none"], 3, 1)
NO_TAIL = ([2, 64, 16], ["relu", "none"], 4, 0)


@pytest.fixture(scope="module")
def ext():
    from nn_distributed_training_amd.ops import get_ext

    return get_ext()


@pytest.fixture(autouse=True)
def _fp32_default():
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float32)
    torch.manual_seed(11)
    yield
    torch.set_default_dtype(old)


def make_spec(widths, acts, w_off=0):
    rows, off = [], w_off
    for i, o, a in zip(widths, widths[1:], acts):
        rows.append([0, off, off + i * o, i, o, ACT[a], 0])
        off += i * o + o
    scales = torch.full((len(rows),), SCALE, dtype=torch.float64)
    return torch.tensor(rows, dtype=torch.long), scales, off


def make_chain(chain, M):
    widths, acts, w_off, pad = chain
    spec, scales, n = make_spec(widths, acts, w_off)
    theta = chk.uniform(L, n + pad, dev=DEV)
    X = chk.uniform(L * M, widths[0], dev=DEV)
    return spec, scales, theta, X


def sentinels(widths, M):
    return [torch.full((L * M, o), 7.0, device=DEV) for o in widths[1:]]


def check_layers(chain, spec, theta, X, outs, M):
    widths, acts = chain[0], chain[1]
    nl = len(acts)
    tail = nl >= 3 and widths[-1] <= 4
    below = X
    for li, (w_off, b_off, i, o) in enumerate(spec[:, 1:5].tolist()):
        trunk = li > 0 and not (tail and li == nl - 1)
        W = chk.weight(theta, w_off, o, i)
        A, W = (bf(below), bf(W)) if trunk else (below.double(), W.double())
        z = torch.einsum("lmi,loi->lmo", A.reshape(L, M, i), W)
        z = (z + theta[:, None, b_off:b_off + o].double()).reshape(L * M, o)
        torch.testing.assert_close(
            outs[li].double(), ACT_FWD[acts[li]](z), **TOL,
            msg=lambda m, li=li: f"layer {li}: {m}")
        below = outs[li]


@pytest.mark.parametrize(
    "chain,M,max_blocks",
    [
        (FLAGSHIP, 128, 0),  # full tiles, 4 k-steps of 64, tail
        (RAGGED, 130, 0),    # row tail, ragged widths, K tails 8, 8, 24,
                             # odd w_off and n
        (NO_TAIL, 128, 0),   # the chain ends in a trunk layer
        (FLAGSHIP, 321, 1),  # one block: 6 tiles, both nodes (weights
                             # staged again), a 1-row tail tile
    ],
)
def test_layers(ext, chain, M, max_blocks):
    spec, scales, theta, X = make_chain(chain, M)
    assert ext.mlp_fwd_fusable(spec, M, 1, torch.float32)
    outs = sentinels(chain[0], M)
    ext.mlp_fwd_fused(spec, scales, X, theta, outs, M, max_blocks)
    check_layers(chain, spec, theta, X, outs, M)
    if max_blocks == 0 and chain is not NO_TAIL:
        # inference variant: the same output, nothing else written
        y = torch.full_like(outs[-1], 7.0)
        ext.mlp_fwd_fused(spec, scales, X, theta,
                          [None] * (len(outs) - 1) + [y], M)
        assert torch.equal(y, outs[-1])


def test_dispatch(ext):
    M = 128
    spec, scales, theta, X = make_chain(FLAGSHIP, M)
    wide = make_spec([2, 256, 128, 1], ["relu"] * 3)
    deep = make_spec([2] + [16] * 9, ["relu"] * 9)
    f32 = torch.float32
    assert not ext.mlp_fwd_fusable(spec, M, 0, f32)
    assert not ext.mlp_fwd_fusable(spec, 64, 1, f32)
    assert not ext.mlp_fwd_fusable(wide[0], M, 1, f32)
    assert not ext.mlp_fwd_fusable(deep[0], M, 1, f32)
    for sp, sc, n, m in [(spec, scales, 0, 64), (*wide, M), (*deep, M)]:
        th = theta if n == 0 else chk.uniform(L, n, dev=DEV)
        widths = [int(sp[0, 3])] + sp[:, 4].tolist()
        with pytest.raises(RuntimeError):
            ext.mlp_fwd_fused(sp, sc, X[:L * m], th, sentinels(widths, m), m)
    with pytest.raises(RuntimeError):  # neither all buffers nor the last
        outs = sentinels(FLAGSHIP[0], M)
        ext.mlp_fwd_fused(spec, scales, X, theta, [None] + outs[1:], M)

    def chain(*fuse):
        outs = sentinels(FLAGSHIP[0], M)
        none = [None] * len(outs)
        ext.fwd_chain(spec, scales, None, None, 0, 0, X, theta, outs, none,
                      none, None, M, False, 1, *fuse)
        return torch.cat(outs, dim=1)

    assert torch.equal(chain(), chain(0))
    fused = sentinels(FLAGSHIP[0], M)
    ext.mlp_fwd_fused(spec, scales, X, theta, fused, M)
    assert torch.equal(chain(1), torch.cat(fused, dim=1))


def test_engine(ext, monkeypatch):
    """fused_forward: true reaches fwd_chain as fuse = 1 in training and
    validation, the validation pack keeps only the output buffer, and
    the encode stash is the layered bf16 engine's."""
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
    fuse_args = []
    real = ext.fwd_chain
    monkeypatch.setattr(
        ext, "fwd_chain",
        lambda *a: (fuse_args.append(a[-1]), real(*a))[1])

    def engine(fused):
        torch.manual_seed(3)
        conf = {
            "problem_name": "fused", "train_batch_size": B,
            "val_batch_size": B, "verbose_evals": False, "data_seed": 3,
            "metrics": ["consensus_error"], "gemm_precision": "bf16",
            "fused_forward": fused,
            "metrics_config": {"evaluate_frequency": 1000},
            "optimizer_config": {"alg_name": "dsgd"},
        }
        pr = DistDensityProblem(
            nx.path_graph(N), FourierNet([2, 256, 64, 64, 1], scale=0.05),
            torch.nn.BCELoss(), sets[:N], sets[N], DEV, conf,
        )
        eng = StackedEngine(pr)
        xb, _ = eng.next_batch()
        eng.forward(xb)
        return eng

    layered, eng = engine(False), engine(True)
    assert fuse_args == [0, 1]
    torch.testing.assert_close(
        eng._bufs["acts"][0], layered._bufs["acts"][0], **TOL)
    v1, v2 = eng.validate_all(), eng.validate_all()
    assert fuse_args[2:] == [1, 1]
    assert [a is None for a in eng._val_pack["acts"]] == [True] * 3 + [False]
    assert torch.isfinite(v1).all() and torch.equal(v1, v2)
