"""ext.fc_block against torch autograd at the edges of its pipeline.

fc_block_k streams the fc1 forward in 32-column K stages through a
double-buffered LDS stage (FC_DEPTH stages alive at once) and deals
the dX0 pass out in 16-column strips, wave w taking strips w, w+8, ...
through two register slots that reload two strips ahead. The shapes
below are the smallest that reach each edge of both pipelines: a stream
shorter than the prologue, exactly as deep, a last-stage drain, ragged
row tiles, K tails, small H, the maximum C, and strip counts on either
side of a slot reload.
"""

import pytest
import torch

from test_ops_gpu import TOL

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(
    not torch.cuda.is_available(), reason="needs MI355X"
)

FC_DEPTH = 2  # K stages alive at once (fused_mnist.hip P1)

SHAPES = [
    (16, 32, 64, 10),    # one 32-wide K stage, prologue deeper than it
    (16, 32 * FC_DEPTH, 64, 10),  # exactly as many stages as the depth
    (16, 96, 64, 10),    # one stage more than the depth
    (17, 33, 64, 2),     # ragged row tile plus a one-element K tail
    (16, 64 * FC_DEPTH + 32, 64, 10),  # last-stage drain
    (64, 432, 64, 10),   # the fast path (MNIST shape)
    (40, 50, 16, 16),    # small H, maximum C
    (5, 130, 48, 7),     # M < tile, two dX0 chunks + a ragged third
    (16, 8, 64, 10),     # dX0: one strip, 7 waves get none
    (16, 256, 64, 10),   # dX0: 16 strips, both slots used, no reload
    (16, 264, 64, 10),   # dX0: 17 strips, first slot reloads once
    (16, 400, 64, 10),   # dX0: 25 strips, second slot reloads too
]


@pytest.fixture(scope="module")
def ext():
    from nn_distributed_training_amd.ops import get_ext

    return get_ext()


def _fp_tol(dtype):
    return TOL[dtype] if dtype == torch.float64 else dict(
        rtol=1e-3, atol=1e-4)


def _run_and_check(ext, dtype, L, M, I, H, C, mask_dx0=False,
                   with_loss=True):
    torch.manual_seed(6)
    dev = torch.device("cuda")
    n = H * I + H + C * H + C
    w1_off, b1_off = 0, H * I
    w2_off, b2_off = H * I + H, H * I + H + C * H
    theta = torch.randn(L, n, dtype=dtype, device=dev) * 0.3
    x0 = torch.randn(L * M, I, dtype=dtype, device=dev)
    if mask_dx0:
        x0 = torch.relu(x0)
    maxlen = M + 5
    Y_all = torch.randint(0, C, (L, maxlen), device=dev)
    off = 3
    idx = torch.arange(maxlen, device=dev).repeat(L, 1)
    idx = (idx + 1) % maxlen  # non-trivial mapping
    loss_scale = 0.7

    grad = torch.zeros_like(theta)
    dx0 = torch.empty_like(x0)
    dz1g = torch.empty(L * M, H, dtype=dtype, device=dev)
    loss = torch.zeros(L, dtype=dtype, device=dev) if with_loss else None
    ext.fc_block(x0, theta, Y_all, idx, maxlen, off, grad, dx0, dz1g,
                 loss, w1_off, b1_off, w2_off, b2_off, M, I, H, C,
                 loss_scale, mask_dx0)

    tol = _fp_tol(dtype)
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
        ref_dx = xl.grad
        if mask_dx0:
            ref_dx = ref_dx * (xl.detach() > 0)
        if with_loss:
            torch.testing.assert_close(loss[l], ref_loss.detach(), **tol)
        torch.testing.assert_close(dx0[l * M:(l + 1) * M], ref_dx, **tol)
        torch.testing.assert_close(
            grad[l, :H * I].reshape(H, I), W1.grad, **tol)
        torch.testing.assert_close(grad[l, b1_off:b1_off + H],
                                   b1.grad, **tol)
        torch.testing.assert_close(
            grad[l, w2_off:w2_off + C * H].reshape(C, H), W2.grad,
            **tol)
        torch.testing.assert_close(grad[l, b2_off:], b2.grad, **tol)


@requires_gpu
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("L", [1, 3])
@pytest.mark.parametrize("M,I,H,C", SHAPES)
def test_fc_block_pipeline_edges(ext, dtype, L, M, I, H, C):
    _run_and_check(ext, dtype, L, M, I, H, C)


@requires_gpu
@pytest.mark.parametrize("M,I,H,C", [(64, 432, 64, 10), (17, 33, 64, 2)])
def test_fc_block_masked_dx0(ext, M, I, H, C):
    """mask_dx0=True: x0 is a relu output and dx0 carries its mask."""
    _run_and_check(ext, torch.float64, 2, M, I, H, C, mask_dx0=True)


@requires_gpu
def test_fc_block_without_loss(ext):
    """loss=None: gradients only, no loss accumulation."""
    _run_and_check(ext, torch.float64, 2, 64, 432, 64, 10,
                   with_loss=False)
