"""ext.fc_block on its two chip-filling kernels, at the edges of the split.

fc_fwd_split_k cuts the fc1 contraction (K = I) into S slices of whole
4-wide MFMA k-steps per 16-row tile; each slice block writes a partial
z1 slab, draws a ticket, and the last one to arrive sums the slabs in
slice order and runs the fc2 forward, the loss and the fc2 backward.
fc_dx0_k computes dX0 on a grid of 16-column strips of I by 64-row
groups of M. The shapes below are the smallest that reach each edge:
fewer k-steps than slices (empty slices), an I that is no multiple of 4,
an even split, ragged and multiple row tiles, a second 64-row group,
H < 64, one node. The reference is torch autograd on the same inputs,
at the tolerances of test_fc_block_pipeline_gpu.py.
"""

import pytest
import torch

from test_ops_gpu import TOL

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(
    not torch.cuda.is_available(), reason="needs MI355X"
)


@pytest.fixture(scope="module")
def ext():
    from nn_distributed_training_amd.ops import get_ext

    return get_ext()


def _fp_tol(dtype):
    return TOL[dtype] if dtype == torch.float64 else dict(
        rtol=1e-3, atol=1e-4)


def _offsets(I, H, C):
    w1, b1 = 0, H * I
    w2, b2 = H * I + H, H * I + H + C * H
    return w1, b1, w2, b2, b2 + C


def _inputs(seed, dtype, L, M, I, H, C, mask_dx0):
    g = torch.Generator(device="cuda").manual_seed(seed)
    dev = torch.device("cuda")
    n = _offsets(I, H, C)[4]
    theta = torch.randn(L, n, dtype=dtype, device=dev, generator=g) * 0.3
    x0 = torch.randn(L * M, I, dtype=dtype, device=dev, generator=g)
    if mask_dx0:
        x0 = torch.relu(x0)
    maxlen = M + 5
    Y_all = torch.randint(0, C, (L, maxlen), device=dev, generator=g)
    idx = torch.arange(maxlen, device=dev).repeat(L, 1)
    idx = (idx + 1) % maxlen  # non-trivial mapping
    return theta, x0, Y_all, idx, maxlen


OFF = 3
LOSS_SCALE = 0.7


def _call(ext, inp, M, I, H, C, mask_dx0=False, with_loss=True):
    theta, x0, Y_all, idx, maxlen = inp
    L = theta.shape[0]
    w1, b1, w2, b2, _ = _offsets(I, H, C)
    grad = torch.zeros_like(theta)
    dx0 = torch.empty_like(x0)
    dz1g = torch.empty(L * M, H, dtype=x0.dtype, device=x0.device)
    loss = torch.zeros(L, dtype=x0.dtype, device=x0.device) \
        if with_loss else None
    ext.fc_block(x0, theta, Y_all, idx, maxlen, OFF, grad, dx0, dz1g,
                 loss, w1, b1, w2, b2, M, I, H, C, LOSS_SCALE, mask_dx0)
    return grad, dx0, dz1g, loss


def _check(inp, out, M, I, H, C, mask_dx0=False):
    theta, x0, Y_all, idx, _ = inp
    grad, dx0, dz1g, loss = out
    L = theta.shape[0]
    w1_off, b1_off, w2_off, b2_off, _ = _offsets(I, H, C)
    tol = _fp_tol(x0.dtype)
    for l in range(L):
        W1 = theta[l, :H * I].reshape(H, I).detach().requires_grad_()
        b1 = theta[l, b1_off:b1_off + H].detach().requires_grad_()
        W2 = theta[l, w2_off:w2_off + C * H].reshape(C, H) \
            .detach().requires_grad_()
        b2 = theta[l, b2_off:].detach().requires_grad_()
        xl = x0[l * M:(l + 1) * M].detach().requires_grad_()
        tgt = Y_all[l][idx[l, OFF:OFF + M]]
        z1 = xl @ W1.T + b1
        z1.retain_grad()
        z2 = torch.relu(z1) @ W2.T + b2
        ref_loss = torch.nn.functional.nll_loss(
            torch.log_softmax(z2, dim=1), tgt)
        (ref_loss * LOSS_SCALE).backward()
        ref_dx = xl.grad
        if mask_dx0:
            ref_dx = ref_dx * (xl.detach() > 0)
        if loss is not None:
            torch.testing.assert_close(loss[l], ref_loss.detach(), **tol)
        torch.testing.assert_close(dz1g[l * M:(l + 1) * M], z1.grad, **tol)
        torch.testing.assert_close(dx0[l * M:(l + 1) * M], ref_dx, **tol)
        torch.testing.assert_close(
            grad[l, :H * I].reshape(H, I), W1.grad, **tol)
        torch.testing.assert_close(grad[l, b1_off:b1_off + H],
                                   b1.grad, **tol)
        torch.testing.assert_close(
            grad[l, w2_off:w2_off + C * H].reshape(C, H), W2.grad,
            **tol)
        torch.testing.assert_close(grad[l, b2_off:], b2.grad, **tol)


def _run_and_check(ext, dtype, L, M, I, H, C, mask_dx0=False,
                   with_loss=True, seed=6):
    inp = _inputs(seed, dtype, L, M, I, H, C, mask_dx0)
    out = _call(ext, inp, M, I, H, C, mask_dx0, with_loss)
    _check(inp, out, M, I, H, C, mask_dx0)
    return inp, out


@requires_gpu
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("I", [
    4,    # one k-step: every slice but the first is empty
    12,   # three k-steps: fewer than the slices
    20,   # five k-steps: a ragged last slice
    108,  # 27 k-steps: uneven over the slices
    110,  # no multiple of 4: a K tail inside the last k-step
    432,  # the MNIST shape: splits evenly, the guard-free path
])
def test_k_split_edges(ext, dtype, I):
    _run_and_check(ext, dtype, 2, 16, I, 64, 10)


@requires_gpu
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("M", [1, 17, 64, 80])
def test_m_tails(ext, dtype, M):
    """Ragged row tiles; M = 80 gives fc_dx0_k a second 64-row group."""
    _run_and_check(ext, dtype, 2, M, 48, 64, 10)


@requires_gpu
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("mask_dx0", [False, True])
def test_small_h(ext, dtype, mask_dx0):
    """H = 40: the contraction's zero padding up to 64, both kernels."""
    _run_and_check(ext, dtype, 2, 17, 48, 40, 10, mask_dx0=mask_dx0)


@requires_gpu
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_one_node(ext, dtype):
    _run_and_check(ext, dtype, 1, 17, 48, 64, 10, mask_dx0=True)


@requires_gpu
@pytest.mark.parametrize("L", [
    16,  # 64 row tiles x 4 slices = 256 blocks: the last split shape
    17,  # 68 row tiles: past the CU count, the one-launch kernel
])
def test_either_side_of_the_dispatch(ext, L):
    """ext.hip fc_kernel_for: both kernels give the same contract."""
    _run_and_check(ext, torch.float64, L, 64, 48, 64, 10, mask_dx0=True)


@requires_gpu
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_ticket_and_slab_reuse(ext, dtype):
    """Three back-to-back calls, (L, M) changed before the third: a
    ticket left non-zero or a slab read from an earlier call fails its
    own reference."""
    runs = [
        (_inputs(11, dtype, 3, 32, 432, 64, 10, False), 32),
        (_inputs(12, dtype, 3, 32, 432, 64, 10, False), 32),
        (_inputs(13, dtype, 2, 17, 432, 64, 10, False), 17),
    ]
    outs = [_call(ext, inp, M, 432, 64, 10) for inp, M in runs]
    for (inp, M), out in zip(runs, outs):
        _check(inp, out, M, 432, 64, 10)


@requires_gpu
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_order_independence(ext, dtype):
    """Slabs are summed in slice order, so everything downstream of z1
    that does not go through atomics is bit-equal between two calls."""
    M, I, H, C = 64, 432, 64, 10
    inp = _inputs(21, dtype, 4, M, I, H, C, True)
    g1, dx1, dz1, l1 = _call(ext, inp, M, I, H, C, mask_dx0=True)
    g2, dx2, dz2, l2 = _call(ext, inp, M, I, H, C, mask_dx0=True)
    _check(inp, (g1, dx1, dz1, l1), M, I, H, C, mask_dx0=True)
    fc1 = H * I + H
    assert torch.equal(dz1, dz2)
    assert torch.equal(dx1, dx2)
    assert torch.equal(g1[:, :fc1], g2[:, :fc1])
    tol = _fp_tol(dtype)
    torch.testing.assert_close(g1[:, fc1:], g2[:, fc1:], **tol)
    torch.testing.assert_close(l1, l2, **tol)


@requires_gpu
def test_without_loss_buffer(ext):
    """loss=None gives the same gradients as a call with a loss slot."""
    M, I, H, C = 17, 108, 64, 10
    inp = _inputs(31, torch.float64, 2, M, I, H, C, False)
    g1, dx1, dz1, _ = _call(ext, inp, M, I, H, C, with_loss=True)
    g2, dx2, dz2, l2 = _call(ext, inp, M, I, H, C, with_loss=False)
    assert l2 is None
    _check(inp, (g2, dx2, dz2, None), M, I, H, C)
    fc1 = H * I + H
    assert torch.equal(dz1, dz2)
    assert torch.equal(dx1, dx2)
    assert torch.equal(g1[:, :fc1], g2[:, :fc1])
    torch.testing.assert_close(g1[:, fc1:], g2[:, fc1:],
                               **_fp_tol(torch.float64))
