"""bf16 activation storage (ops/hip/gemm_bf16_act.hip) against the fp64
product of the bf16-rounded operands (gemm_bf16_checks). A bf16 output
may be off by half a bf16 ulp (2^-8 relative) on top of TOL."""

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
BF16, F32 = torch.bfloat16, torch.float32
DT = {"bf16": BF16, "fp32": F32}
TOL_BF = dict(rtol=2.0 ** -8 + TOL["rtol"], atol=TOL["atol"])


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


def fwd_case(ext, xt, yt, M, I, O, act, round_ops):
    w_off, b_off = 5, 5 + I * O
    theta = chk.uniform(L, b_off + O, dev=DEV)
    assert theta.shape[1] % 2  # odd n: node 1's W rows are unaligned
    xt, yt = DT[xt], DT[yt]
    X = chk.uniform(L * M, I, dev=DEV).to(xt)
    Y = torch.full((L * M, O), 7.0, device=DEV, dtype=yt)
    ext.linear_fwd(X, theta, Y, None, w_off, b_off, M, I, O, ACT[act], SCALE,
                   1)
    r = bf if round_ops else torch.Tensor.double
    z = torch.einsum("lmi,loi->lmo", r(X).reshape(L, M, I),
                     r(chk.weight(theta, w_off, O, I)))
    z = (z + theta[:, None, b_off:b_off + O].double()).reshape(L * M, O)
    ref = chk.ACT_FWD[act](z) if act != "none" else z
    tol = TOL_BF if yt == BF16 else TOL
    torch.testing.assert_close(Y.double(), ref, **tol)


@pytest.mark.parametrize(
    "xt,yt,M,I,O,act",
    [
        ("bf16", "bf16", 128, 64, 64, "relu"),     # the minimum full tile
        ("bf16", "bf16", 130, 72, 40, "relu"),     # M, K (8), O tails
        ("bf16", "fp32", 192, 256, 64, "sigmoid"),  # 8 k-steps prefetched
        ("fp32", "bf16", 129, 8, 16, "none"),      # minimum I/O
        ("fp32", "bf16", 130, 72, 80, "relu"),     # two o-tiles
    ],
)
def test_fwd(ext, xt, yt, M, I, O, act):
    fwd_case(ext, xt, yt, M, I, O, act, round_ops=True)


@pytest.mark.parametrize(
    "M,I,O,act", [(1024, 2, 256, "sin_relu"), (1025, 3, 64, "relu")])
def test_encode(ext, M, I, O, act):
    # contracts in fp32 on the VALU: unrounded operands
    fwd_case(ext, "fp32", "bf16", M, I, O, act, round_ops=False)


@pytest.mark.parametrize(
    "M,I,O,act,Ib",
    [
        (128, 64, 64, "relu", 0),
        (130, 72, 40, "relu", 0),      # ragged everywhere, K (= O) tail 8
        (192, 256, 64, "relu", 0),     # four i-tiles
        (192, 64, 256, "relu", 0),     # 4 stages
        (128, 64, 64, "sin_relu", 2),  # z recomputed; Yb is not read
    ],
)
def test_dx(ext, M, I, O, act, Ib):
    w_off, wb_off = 3, 3 + O * I
    bb_off = wb_off + I * max(Ib, 1)
    theta = chk.uniform(L, bb_off + I + 2, dev=DEV)
    assert theta.shape[1] % 2
    dZ = chk.uniform(L * M, O, dev=DEV)
    if Ib:
        # linear_bwd_dx wants a Yb for every activation: NaNs, never read
        Xb2 = chk.uniform(L * M, Ib, dev=DEV)
        Yb = torch.full((L * M, I), float("nan"), device=DEV, dtype=BF16)
        zb = torch.einsum("lmj,lij->lmi", Xb2.double().reshape(L, M, Ib),
                          chk.weight(theta, wb_off, I, Ib).double())
        zb = (zb + theta[:, None, bb_off:bb_off + I].double())
        fac = chk.ACT_BWD[act](zb.reshape(L * M, I), None)
    else:
        Xb2, zb = None, chk.uniform(L * M, I, dev=DEV, amp=2.0)
        Yb = torch.relu(zb).to(BF16)
        fac = (Yb > 0).double()
    dX = torch.full((L * M, I), 7.0, device=DEV)
    ext.linear_bwd_dx(dZ, theta, dX, Yb, None, ACT[act], SCALE, w_off, M, I,
                      O, Xb2, wb_off, bb_off, Ib, 1)
    ref = torch.einsum("lmo,loi->lmi", bf(dZ).reshape(L, M, O),
                       bf(chk.weight(theta, w_off, O, I)))
    torch.testing.assert_close(dX.double(), ref.reshape(L * M, I) * fac,
                               **TOL)


def dw_case(ext, M, I, O, gap, xt):
    pad_lo, pad_hi, sentinel = 5, 3, 1000.0  # |dW| <= M/16 < 1000
    torch.manual_seed(9)  # the same inputs on every call
    X = chk.uniform(L * M, I, dev=DEV, amp=0.25).to(xt)
    dZ = chk.uniform(L * M, O, dev=DEV, amp=0.25)
    w_off, b_off = pad_lo, pad_lo + I * O + gap
    end = b_off + O
    g = torch.full((L, end + pad_hi), sentinel, device=DEV)
    assert not ext.dw_accumulates(M, I, O, 1)  # overwrites the sentinel
    ext.linear_bwd_dw(dZ, X, g, w_off, b_off, M, I, O, 1)
    dW = torch.einsum("lmo,lmi->loi", bf(dZ).reshape(L, M, O),
                      bf(X).reshape(L, M, I))
    db = dZ.double().reshape(L, M, O).sum(dim=1)  # dZ unrounded
    ref = torch.cat([dW.reshape(L, O * I), db], dim=1)
    got = torch.cat([g[:, w_off:w_off + I * O], g[:, b_off:end]], dim=1)
    torch.testing.assert_close(got.double(), ref, **TOL)
    assert (g[:, w_off + I * O:b_off] == sentinel).all()
    assert (g[:, :w_off] == sentinel).all() and (g[:, end:] == sentinel).all()
    return g


@pytest.mark.parametrize(
    "M,I,O,gap",  # gap: stack elements between the weights and the bias
    [
        (256, 64, 64, 0),
        (257, 16, 64, 0),    # a chunk of one row
        (300, 256, 64, 0),   # four i-tiles
        (272, 48, 80, 0),    # ragged I, O
        (257, 16, 64, 3),    # separate db slabs
    ],
)
def test_dw(ext, M, I, O, gap):
    dw_case(ext, M, I, O, gap, BF16)


def test_refusals(ext):
    M, I, O = 128, 64, 64
    theta = chk.uniform(L, I * O + O, dev=DEV)
    Xf = chk.uniform(L * M, I, dev=DEV)
    Yb = torch.zeros(L * M, O, device=DEV, dtype=BF16)
    with pytest.raises(RuntimeError, match="Z stash"):
        ext.linear_fwd(Xf, theta, Yb, torch.zeros_like(Xf), 0, I * O, M, I, O,
                       ACT["sin_relu"], SCALE, 1)
    with pytest.raises(RuntimeError, match="sigmoid"):
        ext.linear_bwd_dx(Xf, theta, torch.zeros_like(Xf), Yb, None,
                          ACT["sigmoid"], 1.0, 0, M, I, O, None, 0, 0, 0, 1)


@pytest.mark.parametrize("op", ["fwd", "dx", "dw"])
def test_fp32_calls_untouched(ext, op):
    """Still the gbf16:: kernels (bf16-operand references), same bits."""
    M, I, O, bo = 130, 72, 80, 3 + 72 * 80
    theta = chk.uniform(L, bo + O, dev=DEV)
    A, G = chk.uniform(L * M, I, dev=DEV), chk.uniform(L * M, O, dev=DEV)
    W = bf(chk.weight(theta, 3, O, I))

    def run():
        if op == "dw":
            return dw_case(ext, 272, 48, 80, 0, F32)
        out = torch.full_like(G if op == "fwd" else A, 7.0)
        if op == "fwd":
            ext.linear_fwd(A, theta, out, None, 3, bo, M, I, O, 0, 1.0, 1)
            ref = torch.einsum("lmi,loi->lmo", bf(A).reshape(L, M, I), W)
            ref = ref + theta[:, None, bo:].double()
        else:
            ext.linear_bwd_dx(G, theta, out, None, None, 0, 1.0, 3, M, I, O,
                              None, 0, 0, 0, 1)
            ref = torch.einsum("lmo,loi->lmi", bf(G).reshape(L, M, O), W)
        torch.testing.assert_close(out.double(), ref.reshape(out.shape),
                                   **TOL)
        return out

    assert torch.equal(run(), run())


def test_engine(monkeypatch):
    """Buffer dtypes, C++ chain == python chain bit for bit, gradient error
    vs fp64 autograd at most twice that of gemm_precision: bf16 alone."""
    from torch.nn.utils import parameters_to_vector, vector_to_parameters

    from nn_distributed_training_amd.models import FourierNet
    from nn_distributed_training_amd.ops.stacked import StackedEngine
    from nn_distributed_training_amd.problems import dist_dense_problem

    B, N, shape = 1024, 2, [2, 256, 64, 64, 1]
    sets = [torch.utils.data.TensorDataset(
        torch.rand(B, 2) * 8, torch.randint(0, 2, (B,)).float())
        for _ in range(N + 1)]

    def run(py_chain="0", **extra):
        monkeypatch.setenv("NDTA_PY_CHAIN", py_chain)
        torch.manual_seed(3)
        conf = {"problem_name": "act", "train_batch_size": B,
                "val_batch_size": B, "verbose_evals": False, "data_seed": 3,
                "metrics": ["consensus_error"], "gemm_precision": "bf16",
                "metrics_config": {"evaluate_frequency": 1000},
                "optimizer_config": {"alg_name": "dsgd"}, **extra}
        pr = dist_dense_problem.DistDensityProblem(
            nx.path_graph(N), FourierNet(shape, scale=0.05),
            torch.nn.BCELoss(), sets[:N], sets[N], DEV, conf,
        )
        eng = StackedEngine(pr)
        xb, yb = eng.next_batch()
        eng.fwd_bwd(xb, yb)
        return eng, xb, yb

    old, xb, yb = run()
    new, xb2, _ = run(activation_storage="bf16")
    assert torch.equal(xb, xb2) and torch.equal(old.theta, new.theta)
    assert [a.dtype for a in new._bufs["acts"]] == [BF16, BF16, F32, F32]
    assert torch.equal(new.grad, run("1", activation_storage="bf16")[0].grad)

    net = FourierNet(shape, scale=0.05).double().to(DEV)
    rows = []
    for l in range(N):
        vector_to_parameters(old.theta[l].double(), net.parameters())
        net.zero_grad()
        out = net(xb[l * B:(l + 1) * B].double()).reshape(-1)
        torch.nn.functional.binary_cross_entropy(
            out, yb[l * B:(l + 1) * B].double()).backward()
        rows.append(parameters_to_vector([p.grad for p in net.parameters()]))
    ref = torch.stack(rows)
    e_old = (old.grad.double() - ref).abs().max().item()
    e_new = (new.grad.double() - ref).abs().max().item()
    print(f"e_old = {e_old:.3e}, e_new = {e_new:.3e}")
    assert 0 < e_new <= 2 * e_old
