"""conv_pool_fwd_k: the exact-K (K == KMAX) register-window path and the
guarded K < KMAX path against torch conv2d -> relu -> max_pool2d, the
argmax byte checked without depending on ties, and the index-sourced
entry point against the plain one."""

import pytest
import torch

from test_ops_gpu import TOL

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(
    not torch.cuda.is_available(), reason="needs MI355X"
)

# (L, B, F, K, IMG)
SHAPES = [
    (2, 5, 3, 5, 28),   # the model's shape, small batch
    (1, 1, 1, 5, 12),   # one image, one filter, P=4: 16 items < one wave
    (2, 3, 4, 5, 13),   # conv size 9: last conv row/col never pooled
    (2, 3, 3, 3, 28),   # K < KMAX path
    (1, 2, 2, 7, 28),   # KMAX = 7
]
DTYPES = [torch.float64, torch.float32]


@pytest.fixture(scope="module")
def ext():
    from nn_distributed_training_amd.ops import get_ext

    return get_ext()


def _run(ext, X, theta, B, F, K, IMG):
    P = (IMG - K + 1) // 2
    Y = torch.full((X.shape[0], F * P * P), float("nan"), dtype=X.dtype,
                   device=X.device)
    idx = torch.full((X.shape[0], F * P * P), 255, dtype=torch.uint8,
                     device=X.device)
    ext.conv_pool_fwd(X, theta, Y, idx, 0, F * K * K, B, F, K, IMG)
    return Y, idx


def _reference(X, theta, L, B, F, K, IMG):
    """relu(conv) map [L*B, F, C, C] and its 2x2 max pool, per node."""
    convs = []
    for l in range(L):
        W = theta[l, : F * K * K].reshape(F, 1, K, K)
        b = theta[l, F * K * K:]
        xl = X[l * B:(l + 1) * B].reshape(B, 1, IMG, IMG)
        convs.append(torch.relu(torch.nn.functional.conv2d(xl, W, b)))
    conv = torch.cat(convs)
    return conv, torch.nn.functional.max_pool2d(conv, 2)


@requires_gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("shape", SHAPES)
def test_pooled_output_and_argmax(ext, dtype, shape):
    L, B, F, K, IMG = shape
    torch.manual_seed(11)
    dev = torch.device("cuda")
    P = (IMG - K + 1) // 2
    X = torch.randn(L * B, IMG * IMG, dtype=dtype, device=dev)
    theta = torch.randn(L, F * K * K + F, dtype=dtype, device=dev) * 0.2
    Y, idx = _run(ext, X, theta, B, F, K, IMG)
    conv, pooled = _reference(X, theta, L, B, F, K, IMG)

    Yr = Y.reshape(L * B, F, P, P)
    torch.testing.assert_close(Yr, pooled, **TOL[dtype])

    # the position idx names holds the pooled value (no tie dependence)
    ir = idx.reshape(L * B, F, P, P).long()
    assert int(ir.max()) <= 3
    py = torch.arange(P, device=dev).view(1, 1, P, 1)
    px = torch.arange(P, device=dev).view(1, 1, 1, P)
    cy = 2 * py + (ir >> 1)
    cx = 2 * px + (ir & 1)
    C = conv.shape[-1]
    at_idx = conv.reshape(L * B, F, C * C).gather(
        2, (cy * C + cx).reshape(L * B, F, P * P)
    ).reshape(L * B, F, P, P)
    torch.testing.assert_close(at_idx, Yr, **TOL[dtype])


@requires_gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("K", [5, 3])
def test_all_nonpositive_windows(ext, dtype, K):
    L, B, F, IMG = 2, 3, 3, 28
    torch.manual_seed(12)
    dev = torch.device("cuda")
    X = torch.rand(L * B, IMG * IMG, dtype=dtype, device=dev)
    theta = -torch.rand(L, F * K * K + F, dtype=dtype, device=dev) - 0.01
    Y, idx = _run(ext, X, theta, B, F, K, IMG)
    assert torch.equal(Y, torch.zeros_like(Y))
    assert torch.equal(idx, torch.zeros_like(idx))


@requires_gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("K", [5, 3])
def test_index_sourced_matches_gathered_batch(ext, dtype, K):
    L, B, F, IMG = 2, 5, 3, 28
    maxlen, idx_off, idx_stride = 11, 3, 16
    torch.manual_seed(13)
    dev = torch.device("cuda")
    P = (IMG - K + 1) // 2
    X_all = torch.randn(L, maxlen, IMG * IMG, dtype=dtype, device=dev)
    theta = torch.randn(L, F * K * K + F, dtype=dtype, device=dev) * 0.2
    # a non-identity stream: reversed-ish, repeated rows, different per node
    stream = torch.stack([
        torch.randperm(maxlen, device=dev).repeat(2)[:idx_stride]
        for _ in range(L)
    ]).contiguous()
    rows = stream[:, idx_off:idx_off + B]
    assert not torch.equal(rows, torch.arange(B, device=dev).expand(L, B))
    Xb = torch.stack([X_all[l, rows[l]] for l in range(L)]).reshape(
        L * B, IMG * IMG).contiguous()
    Y, idx = _run(ext, Xb, theta, B, F, K, IMG)

    Y2 = torch.full_like(Y, float("nan"))
    idx2 = torch.full_like(idx, 255)
    ext.conv_pool_fwd_idx(X_all, stream.reshape(-1), idx_stride, idx_off,
                          theta, Y2, idx2, 0, F * K * K, B, F, K, IMG)
    assert Y2.shape == (L * B, F * P * P)
    assert torch.equal(Y2, Y)
    assert torch.equal(idx2, idx)
