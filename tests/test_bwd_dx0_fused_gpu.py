"""The merged backward with dX0 folded in (ext.dw_dx0_conv_bwd_idx).

On its fused path one launch computes fc1 dW/db, each 16-column strip of
dX0 = (dz1 @ W1) * relu'(x0), and the conv dW/db that dX0 feeds; dX0
never reaches memory. The reference builds dX0 in torch and runs the two
entry points the launch replaces (ext.linear_bwd_dw,
ext.conv_pool_bwd_idx) on a sentinel-filled grad stack, indexed as in
test_merged_bwd_gpu.py.

Input scale: W1 ~ 0.3 N(0, 1) and dz1 ~ 0.1 N(0, 1), so a dX0 value is
about 0.2 and a conv dW entry (a sum over M * P * P items) about 20 at
the model's shape. One item lost or doubled moves an entry by ~0.2,
four orders of magnitude above TOL at either precision, while fp32
rounding of the 9,216-term sums (~1e-6 absolute) stays well inside it.
"""

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


def _layout(F, K, IMG, H):
    P = (IMG - (K - 1)) // 2
    I = F * P * P
    cw_off, cb_off = 0, F * K * K
    w1_off = cb_off + F
    b1_off = w1_off + H * I
    rest = b1_off + H            # stands for the fc2 slice
    return I, cw_off, cb_off, w1_off, b1_off, rest, rest + 50


def _elem(dtype):
    return torch.empty((), dtype=dtype).element_size()


def _run_case(ext, dtype, L, M, F, K, IMG, H, fused):
    torch.manual_seed(9)
    dev = torch.device("cuda")
    I, cw_off, cb_off, w1_off, b1_off, rest, n = _layout(F, K, IMG, H)
    maxlen, S, off = M + 7, 2 * M + 3, 2
    assert ext.bwd_dx0_fused_for(L, M, I, H, F, K, IMG,
                                 _elem(dtype)) == fused

    theta = torch.randn(L, n, dtype=dtype, device=dev) * 0.3
    dz1 = torch.randn(L * M, H, dtype=dtype, device=dev) * 0.1
    x0 = torch.relu(torch.randn(L * M, I, dtype=dtype, device=dev))
    pidx = torch.randint(0, 4, (L * M, I), device=dev).to(torch.uint8)
    X_all = torch.randn(L, maxlen, IMG * IMG, dtype=dtype, device=dev)
    src = torch.randint(0, maxlen, (L, S), device=dev)

    def fresh():
        g = torch.full((L, n), SENTINEL, dtype=dtype, device=dev)
        g[:, cw_off:w1_off] = 0  # the conv slice accumulates atomically
        return g

    W1 = theta[:, w1_off:b1_off].reshape(L, H, I)
    dY = torch.bmm(dz1.view(L, M, H), W1).reshape(L * M, I) * (x0 > 0)
    ref = fresh()
    ext.linear_bwd_dw(dz1, x0, ref, w1_off, b1_off, M, I, H)
    ext.conv_pool_bwd_idx(dY, pidx, X_all, src, S, off, ref, cw_off,
                          cb_off, M, F, K, IMG)
    out = fresh()
    ext.dw_dx0_conv_bwd_idx(dz1, x0, theta, pidx, X_all, src, S, off,
                            out, w1_off, b1_off, M, I, H, cw_off, cb_off,
                            F, K, IMG)

    # fc1 dW/db: a store path with an unchanged summation order
    assert torch.equal(out[:, w1_off:rest], ref[:, w1_off:rest])
    assert not (ref[:, w1_off:rest] == SENTINEL).any()
    # conv dW/db: atomics, and dX0 from the MFMA not from torch
    torch.testing.assert_close(out[:, cw_off:w1_off],
                               ref[:, cw_off:w1_off], **TOL[dtype])
    assert ref[:, cw_off:w1_off].abs().max() > 0
    assert out[:, cw_off:w1_off].abs().max() > 0
    # everything else is untouched
    assert (out[:, rest:] == SENTINEL).all()


@requires_gpu
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("L,M,F,K,IMG,H", [
    (2, 5, 2, 5, 12, 50),   # P=4: one strip per filter; three waves
                            # without rows; H < 64 padding
    (3, 17, 2, 5, 12, 64),  # ragged second wave
    (2, 64, 3, 5, 28, 50),  # the model's layer shape
    (1, 80, 2, 7, 14, 40),  # second row group; K = 7
])
def test_fused_matches_separate(ext, dtype, L, M, F, K, IMG, H):
    _run_case(ext, dtype, L, M, F, K, IMG, H, fused=True)


@requires_gpu
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_fallback_matches_separate(ext, dtype):
    """P = 3: a strip would straddle filters, so fc_dx0_k writes a
    scratch dX0 and dw_conv_bwd_idx reads it."""
    _run_case(ext, dtype, 3, 5, 2, 3, 8, 48, fused=False)


@requires_gpu
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_fwd_bwd_leaves_dx0_alone(ext, dtype):
    """ext.mnist_fwd_bwd on the fused path never touches dx0, and gives
    the grad stack of ext.fc_block + ext.dw_conv_bwd_idx."""
    torch.manual_seed(4)
    dev = torch.device("cuda")
    L, M, F, K, IMG, H, C = 2, 16, 3, 5, 28, 64, 10
    I, cw_off, cb_off, w1_off, b1_off, w2_off, _ = _layout(F, K, IMG, H)
    b2_off = w2_off + C * H
    n = b2_off + C
    maxlen, S, off = M + 7, 2 * M + 3, 2
    assert ext.bwd_dx0_fused_for(L, M, I, H, F, K, IMG, _elem(dtype))

    theta = torch.randn(L, n, dtype=dtype, device=dev) * 0.3
    X_all = torch.randn(L, maxlen, IMG * IMG, dtype=dtype, device=dev)
    Y_all = torch.randint(0, C, (L, maxlen), device=dev)
    src = torch.randint(0, maxlen, (L, S), device=dev)

    def bufs():
        return dict(
            x0=torch.empty(L * M, I, dtype=dtype, device=dev),
            pidx=torch.empty(L * M, I, dtype=torch.uint8, device=dev),
            grad=torch.zeros(L, n, dtype=dtype, device=dev),
            dx0=torch.full((L * M, I), SENTINEL, dtype=dtype, device=dev),
            dz1=torch.empty(L * M, H, dtype=dtype, device=dev),
            loss=torch.zeros(L, dtype=dtype, device=dev),
        )

    a = bufs()
    ext.mnist_fwd_bwd(X_all, src, S, off, theta, Y_all, a["x0"],
                      a["pidx"], a["grad"], a["dx0"], a["dz1"], a["loss"],
                      cw_off, cb_off, F, K, IMG, w1_off, b1_off, w2_off,
                      b2_off, M, I, H, C, 0.7)
    b = bufs()
    ext.conv_pool_fwd_idx(X_all, src, S, off, theta, b["x0"], b["pidx"],
                          cw_off, cb_off, M, F, K, IMG)
    ext.fc_block(b["x0"], theta, Y_all, src, S, off, b["grad"], b["dx0"],
                 b["dz1"], b["loss"], w1_off, b1_off, w2_off, b2_off, M, I,
                 H, C, 0.7, True)
    ext.dw_conv_bwd_idx(b["dz1"], b["x0"], b["dx0"], b["pidx"], X_all,
                        src, S, off, b["grad"], w1_off, b1_off, M, I, H,
                        cw_off, cb_off, F, K, IMG)

    assert (a["dx0"] == SENTINEL).all()
    assert not (b["dx0"] == SENTINEL).any()
    assert torch.equal(a["x0"], b["x0"])
    assert torch.equal(a["pidx"], b["pidx"])
    assert torch.equal(a["dz1"], b["dz1"])
    ga, gb = a["grad"], b["grad"]
    assert torch.equal(ga[:, w1_off:w2_off], gb[:, w1_off:w2_off])
    torch.testing.assert_close(ga[:, cw_off:w1_off], gb[:, cw_off:w1_off],
                               **TOL[dtype])
    torch.testing.assert_close(ga[:, w2_off:], gb[:, w2_off:],
                               **TOL[dtype])
    assert gb[:, cw_off:w1_off].abs().max() > 0
    assert gb[:, w2_off:].abs().max() > 0
