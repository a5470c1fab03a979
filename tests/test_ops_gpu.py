"""Numerics tests for every CDNA4 kernel vs plain PyTorch references.

All marked @pytest.mark.gpu (run on an MI355X via gpurun / the driver).
Each kernel is compared against an eager fp64 torch computation of the
same op (and again in fp32 with looser tolerance).
"""

import math

import pytest
import torch

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(
    not torch.cuda.is_available(), reason="needs MI355X"
)

TOL = {torch.float64: dict(rtol=1e-10, atol=1e-10),
       torch.float32: dict(rtol=2e-4, atol=2e-5)}


@pytest.fixture(scope="module")
def ext():
    from nn_distributed_training_amd.ops import get_ext

    return get_ext()


def _dev():
    return torch.device("cuda")


@requires_gpu
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("act,actname", [(0, "none"), (1, "relu"),
                                          (3, "sigmoid"), (4, "tanh")])
def test_linear_fwd(ext, dtype, act, actname):
    torch.manual_seed(0)
    L, M, I, O, n = 3, 33, 37, 19, 37 * 19 + 19
    dev = _dev()
    X = torch.randn(L * M, I, dtype=dtype, device=dev)
    theta = torch.randn(L, n, dtype=dtype, device=dev)
    Y = torch.empty(L * M, O, dtype=dtype, device=dev)
    ext.linear_fwd(X, theta, Y, None, 0, I * O, M, I, O, act, 1.0)
    for l in range(L):
        W = theta[l, : I * O].reshape(O, I)
        b = theta[l, I * O :]
        Z = X[l * M : (l + 1) * M] @ W.T + b
        ref = {
            "none": Z, "relu": torch.relu(Z),
            "sigmoid": torch.sigmoid(Z), "tanh": torch.tanh(Z),
        }[actname]
        torch.testing.assert_close(
            Y[l * M : (l + 1) * M], ref, **TOL[dtype]
        )


@requires_gpu
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("M", [40, 2048])  # tiled vs small-K kernels
def test_linear_fwd_sin_relu(ext, dtype, M):
    """FourierNet encode: relu(sin(scale * (Wx+b))) with Z saved."""
    torch.manual_seed(1)
    L, I, O = 2, 2, 24
    n = I * O + O
    dev = _dev()
    scale = 0.05
    X = torch.randn(L * M, I, dtype=dtype, device=dev)
    theta = torch.randn(L, n, dtype=dtype, device=dev)
    Y = torch.empty(L * M, O, dtype=dtype, device=dev)
    Z = torch.empty_like(Y)
    ext.linear_fwd(X, theta, Y, Z, 0, I * O, M, I, O, 2, scale)
    for l in range(L):
        W = theta[l, : I * O].reshape(O, I)
        b = theta[l, I * O :]
        z = X[l * M : (l + 1) * M] @ W.T + b
        ref = torch.relu(torch.sin(scale * z))
        torch.testing.assert_close(Y[l * M : (l + 1) * M], ref,
                                   **TOL[dtype])
        torch.testing.assert_close(Z[l * M : (l + 1) * M], z,
                                   **TOL[dtype])


@requires_gpu
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize(
    "I,O",  # O%64==0 -> register-resident encode_fwd_k; else smallk
    [(2, 256), (3, 64), (2, 100), (4, 128)],
)
def test_linear_fwd_encode_routes(ext, dtype, I, O):
    """Small-K forward at shapes hitting the register-resident encode
    kernel (O a multiple of 64) and the LDS smallk fallback (ragged
    O), with and without the Z stash."""
    torch.manual_seed(2)
    L, M = 3, 2048
    n = I * O + O
    dev = _dev()
    scale = 0.05
    X = torch.randn(L * M, I, dtype=dtype, device=dev)
    theta = torch.randn(L, n, dtype=dtype, device=dev)
    for with_z in (False, True):
        Y = torch.empty(L * M, O, dtype=dtype, device=dev)
        Z = torch.empty_like(Y) if with_z else None
        ext.linear_fwd(X, theta, Y, Z, 0, I * O, M, I, O, 2, scale)
        for l in range(L):
            W = theta[l, : I * O].reshape(O, I)
            b = theta[l, I * O :]
            z = X[l * M : (l + 1) * M] @ W.T + b
            ref = torch.relu(torch.sin(scale * z))
            torch.testing.assert_close(
                Y[l * M : (l + 1) * M], ref, **TOL[dtype]
            )
            if with_z:
                torch.testing.assert_close(
                    Z[l * M : (l + 1) * M], z, **TOL[dtype]
                )


@requires_gpu
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize(
    "L,M,I,O",
    [
        (2, 29, 23, 17),     # VALU path (M < 32)
        (2, 150, 70, 40),    # MFMA fwd/dx/dw with ragged edges
        (2, 4096, 24, 2),    # dw_skinny_o path (O <= 4, big M)
        (1, 4096, 2, 200),   # dw_skinny_i path (generic)
        (1, 4096, 2, 256),   # dw_skinny_i_exact (encode shape I=2 O=256)
        (1, 4096, 17, 9),    # dw_small_chunked fallback
        (1, 4096, 64, 48),   # MFMA dw chunked accumulation + fused db
        (2, 4096, 64, 64),   # dw_direct full-I (density 64->64 shape)
        (1, 4096, 256, 64),  # dw_direct NIMAX=4 (density 256->64)
        (1, 2048, 432, 64),  # dw_direct NIMAX=7 (MNIST fc1 shape)
        (1, 4101, 64, 64),   # dw_direct ragged m-tail (<4 rows)
        (1, 300, 128, 64),   # dw_direct small-M multi-chunk
    ],
)
def test_linear_bwd(ext, dtype, L, M, I, O):
    """dX / dW / db against autograd on y = relu(x @ W^T + b)."""
    torch.manual_seed(2)
    n = I * O + O
    # long reductions accumulate rounding (and the chunked paths add in
    # a different order than torch) — scale tolerance with M
    tol = dict(TOL[dtype])
    if M > 256:
        tol = (
            dict(rtol=3e-3, atol=3e-3)
            if dtype == torch.float32
            else dict(rtol=1e-8, atol=1e-8)
        )
    dev = _dev()
    X = torch.randn(L * M, I, dtype=dtype, device=dev, requires_grad=True)
    theta = torch.randn(L, n, dtype=dtype, device=dev)
    dY = torch.randn(L * M, O, dtype=dtype, device=dev)

    # kernel path
    Y = torch.empty(L * M, O, dtype=dtype, device=dev)
    ext.linear_fwd(X.detach(), theta, Y, None, 0, I * O, M, I, O, 1, 1.0)
    dZ = torch.empty_like(dY)
    ext.act_grad(dY, Y, None, dZ, 1, 1.0)
    dX = torch.empty(L * M, I, dtype=dtype, device=dev)
    ext.linear_bwd_dx(dZ, theta, dX, None, None, 0, 1.0, 0, M, I, O,
                      None, 0, 0, 0)
    gstack = torch.zeros_like(theta)
    ext.linear_bwd_dw(dZ, X.detach(), gstack, 0, I * O, M, I, O)

    # autograd reference per node
    for l in range(L):
        W = theta[l, : I * O].reshape(O, I).detach().requires_grad_()
        b = theta[l, I * O :].detach().requires_grad_()
        xl = X[l * M : (l + 1) * M].detach().requires_grad_()
        y = torch.relu(xl @ W.T + b)
        y.backward(dY[l * M : (l + 1) * M])
        torch.testing.assert_close(dX[l * M : (l + 1) * M], xl.grad,
                                   **tol)
        torch.testing.assert_close(
            gstack[l, : I * O].reshape(O, I), W.grad, **tol
        )
        torch.testing.assert_close(gstack[l, I * O :], b.grad,
                                   **tol)


@requires_gpu
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize(
    "M,I,O",
    [   # one shape on each side of each dW dispatch boundary
        (255, 16, 16),    # small
        (256, 16, 16),    # MFMA
        (256, 16, 64),    # direct
        (256, 18, 16),    # MFMA, I not a multiple of 16
        (2048, 8, 8),     # small
        (2049, 8, 8),     # small-chunked
        (2049, 2, 256),   # skinny-I exact
        (2049, 3, 32),    # skinny-I
        (2049, 32, 2),    # skinny-O
    ],
)
def test_dw_accumulates_matches_kernel(ext, dtype, M, I, O):
    """dw_accumulates() is the zeroing precondition of linear_bwd_dw:
    where it is false the kernel overwrites a sentinel-filled slice,
    where it is true a zeroed slice ends at the same reference; the
    rest of the row is never touched.

    Inputs are uniform in [-0.25, 0.25]: an M-term fp32 sum of their
    products (std 1/48 each) then carries at most about
    6e-8 * (M / sqrt(2)) / 48 = 1.8e-6 of rounding error at M = 2049
    even summed strictly in sequence, 10x under TOL's fp32 atol, while
    the sums themselves (std 0.94) are far above it. The reference is
    the fp64 einsum of the dtype-rounded inputs."""
    L, pad_lo, pad_hi, sentinel = 2, 64, 7, 1000.0  # |dW| <= M/16 < 1000
    acc = ext.dw_accumulates(M, I, O)
    # the rule the stacked engine used before it asked the extension
    assert acc == ((M >= 256 and I >= 16 and O >= 16) or M > 2048)
    torch.manual_seed(5)
    dev = _dev()
    X = (torch.rand(L * M, I, device=dev) * 0.5 - 0.25).to(dtype)
    dZ = (torch.rand(L * M, O, device=dev) * 0.5 - 0.25).to(dtype)
    w_off, b_off = pad_lo, pad_lo + I * O
    end = b_off + O
    g = torch.full((L, end + pad_hi), sentinel, dtype=dtype, device=dev)
    if acc:
        g[:, w_off:end].zero_()
    ext.linear_bwd_dw(dZ, X, g, w_off, b_off, M, I, O)

    dz3 = dZ.double().reshape(L, M, O)
    dW = torch.einsum("lmo,lmi->loi", dz3, X.double().reshape(L, M, I))
    ref = torch.cat([dW.reshape(L, O * I), dz3.sum(dim=1)], dim=1)
    got = g[:, w_off:end]
    print(f"dw {M}x{I}x{O} {dtype} acc={acc} max|err| = "
          f"{(got.double() - ref).abs().max().item():.3e}")
    torch.testing.assert_close(got, ref.to(dtype), **TOL[dtype])
    assert (g[:, :w_off] == sentinel).all()
    assert (g[:, end:] == sentinel).all()


@requires_gpu
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("K", [3, 5, 7])
def test_conv_pool_fwd_bwd(ext, dtype, K):
    # K=5/7 hit the exact KMAX template instantiations; K=3 exercises
    # the K < KMAX case (early-broken unrolled loops, KMAX-strided
    # register accumulators)
    torch.manual_seed(3)
    L, B, F, IMG = 2, 5, 3, 28
    P = (IMG - K + 1) // 2
    n = F * K * K + F
    dev = _dev()
    X = torch.randn(L * B, IMG * IMG, dtype=dtype, device=dev)
    theta = torch.randn(L, n, dtype=dtype, device=dev) * 0.2
    Y = torch.empty(L * B, F * P * P, dtype=dtype, device=dev)
    idx = torch.empty(L * B, F * P * P, dtype=torch.uint8, device=dev)
    ext.conv_pool_fwd(X, theta, Y, idx, 0, F * K * K, B, F, K, IMG)

    dY = torch.randn_like(Y)
    dZ = torch.empty_like(dY)
    ext.act_grad(dY, Y, None, dZ, 1, 1.0)  # relu mask on pooled output
    gstack = torch.zeros_like(theta)
    ext.conv_pool_bwd(dZ, idx, X, gstack, 0, F * K * K, B, F, K, IMG)

    for l in range(L):
        W = (
            theta[l, : F * K * K]
            .reshape(F, 1, K, K)
            .detach()
            .requires_grad_()
        )
        b = theta[l, F * K * K :].detach().requires_grad_()
        xl = X[l * B : (l + 1) * B].reshape(B, 1, IMG, IMG)
        y = torch.nn.functional.max_pool2d(
            torch.relu(torch.nn.functional.conv2d(xl, W, b)), 2
        )
        torch.testing.assert_close(
            Y[l * B : (l + 1) * B].reshape(B, F, P, P), y, **TOL[dtype]
        )
        y.backward(dY[l * B : (l + 1) * B].reshape(B, F, P, P))
        torch.testing.assert_close(
            gstack[l, : F * K * K].reshape(F, 1, K, K), W.grad,
            **TOL[dtype]
        )
        torch.testing.assert_close(gstack[l, F * K * K :], b.grad,
                                   **TOL[dtype])


@requires_gpu
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_logsoftmax_nll(ext, dtype):
    torch.manual_seed(4)
    L, B, C = 3, 16, 10
    M = L * B
    dev = _dev()
    Z = torch.randn(M, C, dtype=dtype, device=dev)
    P = torch.empty_like(Z)
    ext.logsoftmax(Z, P, C)
    torch.testing.assert_close(P, torch.log_softmax(Z, dim=1),
                               **TOL[dtype])

    y = torch.randint(0, C, (M,), device=dev)
    dZ = torch.empty_like(Z)
    loss = torch.zeros(L, dtype=dtype, device=dev)
    ext.nll_bwd(P, y, dZ, loss, C, B, 1.0)

    for l in range(L):
        zl = Z[l * B : (l + 1) * B].detach().requires_grad_()
        ref_loss = torch.nn.functional.nll_loss(
            torch.log_softmax(zl, dim=1), y[l * B : (l + 1) * B]
        )
        ref_loss.backward()
        torch.testing.assert_close(dZ[l * B : (l + 1) * B], zl.grad,
                                   **TOL[dtype])
        torch.testing.assert_close(loss[l], ref_loss.detach(),
                                   **TOL[dtype])


@requires_gpu
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_nll_fused(ext, dtype):
    """Fused logits->LSE->resident-target-gather->dZ kernel vs torch."""
    torch.manual_seed(14)
    L, B, C, maxlen, S = 2, 16, 10, 40, 64
    M = L * B
    dev = _dev()
    Z = torch.randn(M, C, dtype=dtype, device=dev)
    Y_all = torch.randint(0, C, (L, maxlen), device=dev)
    stream = torch.randint(0, maxlen, (L, S), device=dev)
    off = 7
    dZ = torch.empty_like(Z)
    loss = torch.zeros(L, dtype=dtype, device=dev)
    ext.nll_fused(Z, Y_all, stream, dZ, loss, None, 0, S, off, C, B,
                  1.0)

    ar = torch.arange(L, device=dev).unsqueeze(1)
    y = Y_all[ar, stream[:, off : off + B]].reshape(-1)
    for l in range(L):
        zl = Z[l * B : (l + 1) * B].detach().requires_grad_()
        ref = torch.nn.functional.nll_loss(
            torch.log_softmax(zl, dim=1), y[l * B : (l + 1) * B]
        )
        ref.backward()
        torch.testing.assert_close(dZ[l * B : (l + 1) * B], zl.grad,
                                   **TOL[dtype])
        torch.testing.assert_close(loss[l], ref.detach(), **TOL[dtype])

    # device-offset form (hipGraph mode) must agree
    offs_dev = torch.tensor([off], device=dev)
    dZ2 = torch.empty_like(Z)
    ext.nll_fused(Z, Y_all, stream, dZ2, None, offs_dev, 0, S, 0, C, B,
                  1.0)
    torch.testing.assert_close(dZ2, dZ, rtol=0, atol=0)


@requires_gpu
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_bce_bwd(ext, dtype):
    torch.manual_seed(5)
    L, B = 2, 32
    M = L * B
    dev = _dev()
    z = torch.randn(M, dtype=dtype, device=dev)
    p = torch.sigmoid(z)
    t = torch.randint(0, 2, (M,), device=dev).to(dtype)
    dZ = torch.empty_like(z)
    loss = torch.zeros(L, dtype=dtype, device=dev)
    ext.bce_bwd(p, t, dZ, loss, B, 1.0)
    for l in range(L):
        zl = z[l * B : (l + 1) * B].detach().requires_grad_()
        ref = torch.nn.functional.binary_cross_entropy(
            torch.sigmoid(zl), t[l * B : (l + 1) * B]
        )
        ref.backward()
        torch.testing.assert_close(dZ[l * B : (l + 1) * B], zl.grad,
                                   **TOL[dtype])
        torch.testing.assert_close(loss[l], ref.detach(), **TOL[dtype])


@requires_gpu
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_dinno_dual_threg(ext, dtype):
    torch.manual_seed(6)
    L, n, R = 3, 101, 5
    dev = _dev()
    table = torch.randn(R, n, dtype=dtype, device=dev)
    local = table[:L].contiguous()
    remote = table[L:].contiguous()
    # node 0 -> rows {1, 3}; node 1 -> rows {0, 4}; node 2 -> {}
    offs = torch.tensor([0, 2, 4, 4], dtype=torch.int32, device=dev)
    idx = torch.tensor([1, 3, 0, 4], dtype=torch.int32, device=dev)
    duals = torch.randn(L, n, dtype=dtype, device=dev)
    duals0 = duals.clone()
    s = torch.empty_like(duals)
    rho = 0.37
    ext.dinno_dual_threg(local, remote, offs, idx, duals, s, rho)

    nbrs = [[1, 3], [0, 4], []]
    for l in range(L):
        th = table[l]
        S = sum((table[j] for j in nbrs[l]), torch.zeros_like(th))
        deg = len(nbrs[l])
        torch.testing.assert_close(
            duals[l], duals0[l] + rho * (deg * th - S), **TOL[dtype]
        )
        torch.testing.assert_close(s[l], (deg * th + S) / 2, **TOL[dtype])


@requires_gpu
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_mix_and_dsgt_kernels(ext, dtype):
    torch.manual_seed(7)
    L, n, R = 2, 77, 4
    dev = _dev()
    table = torch.randn(R, n, dtype=dtype, device=dev)
    local = table[:L].contiguous()
    remote = table[L:].contiguous()
    offs = torch.tensor([0, 3, 5], dtype=torch.int32, device=dev)
    idx = torch.tensor([0, 2, 3, 1, 2], dtype=torch.int32, device=dev)
    w = torch.randn(5, dtype=dtype, device=dev)
    out = torch.empty(L, n, dtype=dtype, device=dev)
    ext.mix_rows(local, remote, offs, idx, w, out)
    ref0 = w[0] * table[0] + w[1] * table[2] + w[2] * table[3]
    ref1 = w[3] * table[1] + w[4] * table[2]
    torch.testing.assert_close(out[0], ref0, **TOL[dtype])
    torch.testing.assert_close(out[1], ref1, **TOL[dtype])

    # dsgt: local (p, y) stacks + remote [p | y] bundles
    p_loc = torch.randn(L, n, dtype=dtype, device=dev)
    y_loc = torch.randn(L, n, dtype=dtype, device=dev)
    rem2 = torch.randn(R - L, 2 * n, dtype=dtype, device=dev)
    alpha = 0.05
    p_out = torch.empty(L, n, dtype=dtype, device=dev)
    y_mix = torch.empty(L, n, dtype=dtype, device=dev)
    ext.dsgt_mix(p_loc, y_loc, rem2, offs, idx, w, p_out, y_mix, alpha)

    def row_py(r):
        if r < L:
            return p_loc[r], y_loc[r]
        return rem2[r - L, :n], rem2[r - L, n:]

    for l, ks in enumerate([[0, 1, 2], [3, 4]]):
        accp = torch.zeros(n, dtype=dtype, device=dev)
        accy = torch.zeros(n, dtype=dtype, device=dev)
        for k in ks:
            pj, yj = row_py(idx[k].item())
            accp += w[k] * pj
            accy += w[k] * yj
        torch.testing.assert_close(p_out[l], accp - alpha * accy,
                                   **TOL[dtype])
        torch.testing.assert_close(y_mix[l], accy, **TOL[dtype])

    y_mix2 = torch.randn(L, n, dtype=dtype, device=dev)
    g_new = torch.randn(L, n, dtype=dtype, device=dev)
    g_old = torch.randn(L, n, dtype=dtype, device=dev)
    g_old0 = g_old.clone()
    y = torch.empty(L, n, dtype=dtype, device=dev)
    ext.dsgt_y_update(y_mix2, g_new, g_old, y)
    torch.testing.assert_close(y, y_mix2 + g_new - g_old0, **TOL[dtype])
    torch.testing.assert_close(g_old, g_new, **TOL[dtype])


@requires_gpu
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_gather_batch(ext, dtype):
    torch.manual_seed(9)
    L, maxlen, Fdim, B, S = 3, 50, 7, 8, 40
    dev = _dev()
    X = torch.randn(L, maxlen, Fdim, dtype=dtype, device=dev)
    Yt = torch.randint(0, 10, (L, maxlen), device=dev)
    stream = torch.randint(0, maxlen, (L, S), device=dev)
    view = stream[:, 5 : 5 + B]  # strided view (row stride S)
    xb = torch.empty(L * B, Fdim, dtype=dtype, device=dev)
    yb = torch.empty(L * B, dtype=torch.long, device=dev)
    ext.gather_batch(X, view.contiguous(), xb, B, 0)
    ext.gather_targets(Yt, view.contiguous(), yb, B, 0)
    ar = torch.arange(L, device=dev).unsqueeze(1)
    torch.testing.assert_close(
        xb, X[ar, view].reshape(L * B, Fdim), rtol=0, atol=0
    )
    torch.testing.assert_close(
        yb, Yt[ar, view].reshape(-1), rtol=0, atol=0
    )
    # stride+offset form: gather straight out of the stream tensor
    xb2 = torch.empty_like(xb)
    yb2 = torch.empty_like(yb)
    ext.gather_batch(X, stream, xb2, S, 5)
    ext.gather_targets(Yt, stream, yb2, S, 5)
    torch.testing.assert_close(xb2, xb, rtol=0, atol=0)
    torch.testing.assert_close(yb2, yb, rtol=0, atol=0)


@requires_gpu
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("optname,mode", [("adam", 0), ("adamw", 1),
                                           ("sgd", 2)])
def test_fused_step_matches_torch_opt(ext, dtype, optname, mode):
    """Fused DiNNO primal step == autograd loss (reference dinno.py:74-91)
    + torch optimizer, over 3 consecutive steps."""
    torch.manual_seed(8)
    L, n = 2, 53
    dev = _dev()
    theta = torch.randn(L, n, dtype=dtype, device=dev)
    duals = torch.randn(L, n, dtype=dtype, device=dev)
    deg_list = [2, 3]
    th_regs = [
        torch.randn(d, n, dtype=dtype, device=dev) for d in deg_list
    ]
    rho = 0.21
    lr = 0.01
    wd = 0.01 if mode == 1 else 0.0

    # torch reference: replicate primal loss with a fixed "pred grad"
    pred_grad = torch.randn(L, n, dtype=dtype, device=dev)
    ref_params = [theta[l].clone().requires_grad_() for l in range(L)]
    opts = {
        "adam": lambda p: torch.optim.Adam([p], lr),
        "adamw": lambda p: torch.optim.AdamW([p], lr),
        "sgd": lambda p: torch.optim.SGD([p], lr),
    }
    ref_opts = [opts[optname](p) for p in ref_params]

    m = torch.zeros_like(theta)
    v = torch.zeros_like(theta)
    s = torch.stack([
        tr.sum(dim=0) for tr in th_regs
    ])  # placeholder, recomputed below
    deg = torch.tensor(deg_list, dtype=torch.int32, device=dev)

    for step in range(1, 4):
        # s_l = sum_j th_reg_j (constant within a round here)
        for l in range(L):
            s[l] = th_regs[l].sum(dim=0)
        ext.fused_step(
            theta, pred_grad, duals, s, deg,
            None if mode == 2 else m, None if mode == 2 else v,
            rho, lr, 0.9, 0.999, 1e-8, wd, step, mode, step == 1, 1,
            False,
        )
        for l in range(L):
            p = ref_params[l]
            ref_opts[l].zero_grad()
            loss = (
                (pred_grad[l] * p).sum()
                + torch.dot(p, duals[l])
                + rho * torch.sum(
                    torch.square(p.unsqueeze(0) - th_regs[l])
                )
            )
            loss.backward()
            ref_opts[l].step()
            torch.testing.assert_close(theta[l], p.detach(),
                                       **TOL[dtype])


@requires_gpu
def test_feistel_perm(ext):
    """Keyed bijection kernel: permutation of [lb, lb+n), deterministic
    by key, distinct keys give distinct orders (sampler shuffle)."""
    dev = _dev()
    for n in (1, 7, 64, 50000):
        out = torch.empty(n, dtype=torch.long, device=dev)
        ext.feistel_perm(out, n, 100, 12345)
        vals = out.cpu().sort().values
        assert torch.equal(vals, torch.arange(100, 100 + n)), n
    out1 = torch.empty(1000, dtype=torch.long, device=dev)
    out2 = torch.empty(1000, dtype=torch.long, device=dev)
    ext.feistel_perm(out1, 1000, 0, 777)
    ext.feistel_perm(out2, 1000, 0, 777)
    assert torch.equal(out1, out2)
    ext.feistel_perm(out2, 1000, 0, 778)
    assert not torch.equal(out1, out2)
    # not the identity (it actually shuffles)
    assert not torch.equal(out1, torch.arange(1000, device=dev))


@requires_gpu
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("M", [40, 2048])  # VALU vs MFMA dx paths
def test_linear_bwd_dx_sin_relu_recompute(ext, dtype, M):
    """dx with the encode layer's z RECOMPUTED from its tiny input
    (Xb2 @ Wb^T + bb) must match dx with the explicitly stored Zb."""
    torch.manual_seed(5)
    L, Ib, I, O = 2, 2, 24, 16  # below: 2->24 sin_relu; above: 24->16
    dev = _dev()
    scale = 0.05
    nb = Ib * I + I           # below layer params (W1 [I, Ib], b1 [I])
    n = nb + I * O + O        # + above layer
    theta = torch.randn(L, n, dtype=dtype, device=dev)
    Xb2 = torch.randn(L * M, Ib, dtype=dtype, device=dev)

    # below layer forward (explicit z for the reference path)
    Yb = torch.empty(L * M, I, dtype=dtype, device=dev)
    Zb = torch.empty_like(Yb)
    ext.linear_fwd(Xb2, theta, Yb, Zb, 0, Ib * I, M, Ib, I, 2, scale)

    dZ = torch.randn(L * M, O, dtype=dtype, device=dev)
    ref = torch.empty(L * M, I, dtype=dtype, device=dev)
    ext.linear_bwd_dx(dZ, theta, ref, Yb, Zb, 2, scale, nb, M, I, O,
                      None, 0, 0, 0)
    out = torch.empty_like(ref)
    ext.linear_bwd_dx(dZ, theta, out, Yb, None, 2, scale, nb, M, I, O,
                      Xb2, 0, Ib * I, Ib)
    torch.testing.assert_close(out, ref, **TOL[dtype])


@requires_gpu
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("M,I,H,C", [(64, 432, 64, 10),  # MNIST shape
                                     (40, 50, 48, 7)])   # ragged all
def test_fc_block_matches_autograd(ext, dtype, M, I, H, C):
    """One-launch fused fc block (fc1+fc2 fwd, NLL, full fc backward)
    vs torch autograd on the same two-layer head."""
    torch.manual_seed(6)
    L = 2
    dev = _dev()
    n = H * I + H + C * H + C
    w1_off, b1_off = 0, H * I
    w2_off, b2_off = H * I + H, H * I + H + C * H
    theta = torch.randn(L, n, dtype=dtype, device=dev) * 0.3
    x0 = torch.randn(L * M, I, dtype=dtype, device=dev)
    maxlen = M + 5
    Y_all = torch.randint(0, C, (L, maxlen), device=dev)
    # identity-ish index stream with an offset
    off = 3
    idx = torch.arange(maxlen, device=dev).repeat(L, 1)
    idx = (idx + 1) % maxlen  # non-trivial mapping
    loss_scale = 0.7

    grad = torch.zeros_like(theta)
    dx0 = torch.empty_like(x0)
    dz1g = torch.empty(L * M, H, dtype=dtype, device=dev)
    loss = torch.zeros(L, dtype=dtype, device=dev)
    # mask_dx0=False: x0 here is a plain input, not a relu output
    ext.fc_block(x0, theta, Y_all, idx, maxlen, off, grad, dx0, dz1g,
                 loss, w1_off, b1_off, w2_off, b2_off, M, I, H, C,
                 loss_scale, False)

    tol = TOL[dtype] if dtype == torch.float64 else dict(
        rtol=1e-3, atol=1e-4)
    for l in range(L):
        W1 = theta[l, :H * I].reshape(H, I).detach().requires_grad_()
        b1 = theta[l, b1_off:b1_off + H].detach().requires_grad_()
        W2 = theta[l, w2_off:w2_off + C * H].reshape(C, H) \
            .detach().requires_grad_()
        b2 = theta[l, b2_off:].detach().requires_grad_()
        xl = x0[l * M:(l + 1) * M].detach().requires_grad_()
        tgt = Y_all[l][idx[l, off:off + M]]
        y1 = torch.relu(xl @ W1.T + b1)
        z2 = y1 @ W2.T + b2
        ref_loss = torch.nn.functional.nll_loss(
            torch.log_softmax(z2, dim=1), tgt)
        (ref_loss * loss_scale).backward()
        torch.testing.assert_close(loss[l], ref_loss.detach(), **tol)
        torch.testing.assert_close(dx0[l * M:(l + 1) * M], xl.grad,
                                   **tol)
        torch.testing.assert_close(
            grad[l, :H * I].reshape(H, I), W1.grad, **tol)
        torch.testing.assert_close(grad[l, b1_off:b1_off + H],
                                   b1.grad, **tol)
        torch.testing.assert_close(
            grad[l, w2_off:w2_off + C * H].reshape(C, H), W2.grad,
            **tol)
        torch.testing.assert_close(grad[l, b2_off:], b2.grad, **tol)


@requires_gpu
@pytest.mark.parametrize("N,n", [(8, 28440), (3, 100), (32, 25601)])
def test_consensus_cdist_matches_torch(ext, N, n):
    """First-party consensus-error kernels vs the torch reference
    (normalize -> cdist -> cdist-to-mean, reference
    problems/dist_mnist_problem.py:152-175)."""
    torch.manual_seed(8)
    stack = torch.randn(N, n, dtype=torch.float64, device=_dev())
    D, Dm = ext.consensus_cdist(stack)
    ref = torch.nn.functional.normalize(stack, dim=1)
    Dref = torch.cdist(ref, ref)
    Dmref = torch.cdist(ref, ref.mean(dim=0, keepdim=True))
    # torch's mm-based cdist leaves ~1e-7 fuzz on the diagonal (and
    # near-zero entries); the direct-difference kernel is ~1e-17 there
    assert torch.all(D.diagonal().abs() < 1e-12)
    torch.testing.assert_close(D, Dref, rtol=1e-9, atol=5e-7)
    torch.testing.assert_close(Dm, Dmref, rtol=1e-9, atol=5e-7)


@requires_gpu
def test_linear_kernels_randomized_shapes(ext):
    """Seeded random-shape sweep across ALL the linear dispatch
    branches (VALU / MFMA fwd, dx new+old, dw direct/chunked/skinny):
    fwd+dw+db+dx vs autograd at every shape. Guards the many
    shape-routing conditions against edge regressions."""
    import random as _random

    rng = _random.Random(0xC0FFEE)
    torch.manual_seed(11)
    dev = _dev()
    for trial in range(14):
        L = rng.choice([1, 2, 3])
        M = rng.choice([17, 40, 64, 150, 300, 1024, 2600])
        I = rng.choice([2, 3, 16, 17, 48, 64, 70, 128, 256, 333])
        O = rng.choice([1, 2, 5, 10, 17, 40, 64, 128, 200])
        n = I * O + O
        X = torch.randn(L * M, I, dtype=torch.float64, device=dev)
        theta = torch.randn(L, n, dtype=torch.float64, device=dev)
        dY = torch.randn(L * M, O, dtype=torch.float64, device=dev)
        Y = torch.empty(L * M, O, dtype=torch.float64, device=dev)
        ext.linear_fwd(X, theta, Y, None, 0, I * O, M, I, O, 1, 1.0)
        dZ = torch.empty_like(dY)
        ext.act_grad(dY, Y, None, dZ, 1, 1.0)
        dX = torch.empty_like(X)
        ext.linear_bwd_dx(dZ, theta, dX, None, None, 0, 1.0, 0, M, I,
                          O, None, 0, 0, 0)
        g = torch.zeros_like(theta)
        ext.linear_bwd_dw(dZ, X, g, 0, I * O, M, I, O)

        tol = dict(rtol=1e-8, atol=1e-8)
        for l in range(L):
            W = theta[l, : I * O].reshape(O, I).detach() \
                .requires_grad_()
            b = theta[l, I * O:].detach().requires_grad_()
            xl = X[l * M:(l + 1) * M].detach().requires_grad_()
            y = torch.relu(xl @ W.T + b)
            torch.testing.assert_close(Y[l * M:(l + 1) * M], y, **tol)
            y.backward(dY[l * M:(l + 1) * M])
            torch.testing.assert_close(
                dX[l * M:(l + 1) * M], xl.grad, **tol
            ), (trial, L, M, I, O)
            torch.testing.assert_close(
                g[l, : I * O].reshape(O, I), W.grad, **tol
            )
            torch.testing.assert_close(g[l, I * O:], b.grad, **tol)
