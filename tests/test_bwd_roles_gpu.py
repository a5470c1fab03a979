"""The two roles of the merged backward launch, each against a float64
torch reference written here: the conv dW/db reduction (per-wave halving
butterfly over all taps) through all three of its entry points, and the small store-path fc dW/db (64 rows of the
batch staged per pass) through ext.linear_bwd_dw."""

import functools

import pytest
import torch
import torch.nn.functional as Fn

from test_ops_gpu import TOL

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(
    not torch.cuda.is_available(), reason="needs MI355X"
)

SENTINEL = 12345.5
H_FC = 16  # fc1 width handed to the merged launch's dW role

# (L, B, F, K, IMG). Every launcher runs 256-thread blocks and splits a
# (node, filter)'s batch into min(B, 32) chunks of ceil(B / 32) images.
CONV_CASES = [
    # exact-K; 16 items per block, under one wave's worth: idle lanes
    # and idle waves must add zero
    (2, 3, 2, 5, 12),
    # exact-K; one block with 288 items = 256 + 32: wave 0 alone runs a
    # second pass
    (1, 2, 1, 5, 28),
    # exact-K, six one-image chunks of 144 items. A block with more
    # than 2 * nthr items is not reachable this way: no entry point
    # launches fewer than 256 threads; the case below gets there by
    # raising B instead.
    (1, 6, 1, 5, 28),
    # exact-K with work > 2 * 256: 4 images per chunk = 576 items, three
    # passes for wave 0; chunks 25..31 are empty
    (1, 100, 1, 5, 28),
    # KMAX = 7 exact-K; 32 chunks of 2 images, chunks 17..31 are empty
    (2, 33, 2, 7, 10),
    # K < KMAX = 5: skipped taps in the reduction
    (2, 5, 3, 3, 8),
    # K < KMAX = 7
    (1, 4, 2, 6, 12),
]


@pytest.fixture(scope="module")
def ext():
    from nn_distributed_training_amd.ops import get_ext

    return get_ext()


@functools.lru_cache(maxsize=None)
def _conv_case(case, dtype):
    """Seeded inputs of one conv case in `dtype` and the float64
    reference of its [L, F*K*K + F] conv grad slice, computed once and
    shared by the three entry points."""
    L, B, F, K, IMG = case
    dev = torch.device("cuda")
    torch.manual_seed(1234 + 7 * B + K)
    C = IMG - (K - 1)
    P = C // 2
    I = F * P * P
    maxlen, S, off = B + 7, 2 * B + 3, 2

    def randn(*shape):
        return torch.randn(*shape, dtype=dtype, device=dev)

    dY = randn(L * B, I)
    dY = dY * (torch.rand_like(dY) > 0.3)  # relu-masked grads have zeros
    pidx = torch.randint(0, 4, (L * B, I), device=dev).to(torch.uint8)
    X_all = randn(L, maxlen, IMG * IMG)
    src = torch.randint(0, maxlen, (L, S), device=dev)
    rows = src[:, off:off + B]                               # [L, B]
    X = torch.gather(
        X_all, 1, rows[:, :, None].expand(L, B, IMG * IMG)
    ).reshape(L * B, IMG * IMG).contiguous()
    dz1 = randn(L * B, H_FC)
    x0 = torch.relu(randn(L * B, I))

    # reference: pooled grad -> its argmax conv position, then contract
    # with the unfolded image
    g = dY.double().view(L * B, F, P, P)
    d = pidx.long().view(L * B, F, P, P)
    py = torch.arange(P, device=dev).view(1, 1, P, 1)
    px = torch.arange(P, device=dev).view(1, 1, 1, P)
    pos = (2 * py + (d >> 1)) * C + 2 * px + (d & 1)
    G = torch.zeros(L * B, F, C * C, dtype=torch.float64, device=dev)
    G.scatter_add_(2, pos.view(L * B, F, P * P), g.view(L * B, F, P * P))
    patches = Fn.unfold(X.double().view(L * B, 1, IMG, IMG), K)
    dW = torch.einsum("lbfp,lbkp->lfk", G.view(L, B, F, C * C),
                      patches.view(L, B, K * K, C * C))
    db = g.view(L, B, F, P * P).sum(dim=(1, 3))
    ref = torch.cat([dW.reshape(L, F * K * K), db], dim=1)
    return dict(dY=dY, pidx=pidx, X_all=X_all, src=src, S=S, off=off,
                X=X, dz1=dz1, x0=x0, ref=ref)


@requires_gpu
@pytest.mark.parametrize("entry", ["direct", "idx", "merged"])
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("case", CONV_CASES, ids=lambda c: "-".join(
    map(str, c)))
def test_conv_bwd_matches_reference(ext, case, dtype, entry):
    L, B, F, K, IMG = case
    c = _conv_case(case, dtype)
    P = (IMG - (K - 1)) // 2
    I = F * P * P
    cw_off, cb_off = 0, F * K * K
    w1_off = cb_off + F
    b1_off = w1_off + H_FC * I
    rest = b1_off + H_FC
    n = rest + 50
    g = torch.full((L, n), SENTINEL, dtype=dtype, device="cuda")
    g[:, cw_off:w1_off] = 0  # the conv slice accumulates atomically

    if entry == "direct":
        ext.conv_pool_bwd(c["dY"], c["pidx"], c["X"], g, cw_off, cb_off,
                          B, F, K, IMG)
        touched = w1_off
    elif entry == "idx":
        ext.conv_pool_bwd_idx(c["dY"], c["pidx"], c["X_all"], c["src"],
                              c["S"], c["off"], g, cw_off, cb_off, B, F,
                              K, IMG)
        touched = w1_off
    else:
        ext.dw_conv_bwd_idx(c["dz1"], c["x0"], c["dY"], c["pidx"],
                            c["X_all"], c["src"], c["S"], c["off"], g,
                            w1_off, b1_off, B, I, H_FC, cw_off, cb_off,
                            F, K, IMG)
        touched = rest
        assert not (g[:, w1_off:rest] == SENTINEL).any()

    assert c["ref"].abs().max() > 0
    torch.testing.assert_close(g[:, cw_off:w1_off].double(), c["ref"],
                               **TOL[dtype])
    # the rest of the grad stack is untouched
    assert (g[:, touched:] == SENTINEL).all()


@requires_gpu
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("M,I,O", [
    (5, 18, 48),     # edge tiles in all three dimensions
    (64, 432, 64),   # the model's shape: one guard-free pass
    (70, 32, 16),    # a full 64-row pass plus a 6-row pass
    (200, 17, 10),   # four passes, O < 16
])
def test_small_dw_matches_reference(ext, dtype, M, I, O):
    assert not ext.dw_accumulates(M, I, O)  # the Small store path
    torch.manual_seed(4321 + M)
    dev = torch.device("cuda")
    L = 2
    w_off = 3
    b_off = w_off + O * I
    end = b_off + O
    n = end + 9
    dZ = torch.randn(L * M, O, dtype=dtype, device=dev)
    dZ = dZ * (torch.rand_like(dZ) > 0.3)
    X = torch.randn(L * M, I, dtype=dtype, device=dev)
    g = torch.full((L, n), SENTINEL, dtype=dtype, device=dev)
    ext.linear_bwd_dw(dZ, X, g, w_off, b_off, M, I, O)

    dZl = dZ.double().view(L, M, O)
    Xl = X.double().view(L, M, I)
    ref_w = torch.bmm(dZl.transpose(1, 2), Xl).reshape(L, O * I)
    ref_b = dZl.sum(1)
    torch.testing.assert_close(g[:, w_off:b_off].double(), ref_w,
                               **TOL[dtype])
    torch.testing.assert_close(g[:, b_off:end].double(), ref_b,
                               **TOL[dtype])
    # overwritten (no zeroing needed), and nothing else is written
    assert (g[:, :w_off] == SENTINEL).all()
    assert (g[:, end:] == SENTINEL).all()
