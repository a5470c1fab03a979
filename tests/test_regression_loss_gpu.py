"""regression_bwd (MSE / L1 loss head) vs torch.nn.MSELoss / L1Loss.

Per-node mean reduction: node l owns rows [l*B, (l+1)*B) of the stacked
prediction vector, dY is the gradient of loss_scale * loss_l and loss[l]
the unscaled loss_l. B = 37 puts both node boundaries inside a wave.
Inputs are drawn on the CPU, rounded to the test dtype, and the
reference is fp64 autograd on the rounded values.
"""

import pytest
import torch

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(
    not torch.cuda.is_available(), reason="needs MI355X"
)

TOL = {torch.float64: dict(rtol=1e-10, atol=1e-10),
       torch.float32: dict(rtol=2e-4, atol=2e-5)}

SENTINEL = 1000.0
GUARD = 64
SEED = 41
LOSSES = {"mse": (0, torch.nn.MSELoss), "l1": (1, torch.nn.L1Loss)}


@pytest.fixture(scope="module")
def ext():
    from nn_distributed_training_amd.ops import get_ext

    return get_ext()


def _dev():
    return torch.device("cuda")


def _guarded(numel, dtype, fill=SENTINEL):
    buf = torch.full((GUARD + numel + GUARD,), SENTINEL, dtype=dtype,
                     device=_dev())
    buf[GUARD:GUARD + numel] = fill
    return buf, buf[GUARD:GUARD + numel]


def _assert_guards(buf, what):
    assert (buf[:GUARD] == SENTINEL).all(), f"{what}: wrote below range"
    assert (buf[-GUARD:] == SENTINEL).all(), f"{what}: wrote above range"


@requires_gpu
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("kind", ["mse", "l1"])
def test_regression_bwd_matches_torch_loss(ext, dtype, kind):
    mode, loss_cls = LOSSES[kind]
    Lr, B, loss_scale = 3, 37, 0.7
    gen = torch.Generator().manual_seed(SEED)
    yhat = torch.randn(Lr * B, generator=gen,
                       dtype=torch.float64).to(dtype)
    tgt = torch.randn(Lr * B, generator=gen,
                      dtype=torch.float64).to(dtype)
    ties = torch.tensor([0, 36, 37, 63, 64, 110])  # both sides of the
    if kind == "l1":                               # node and wave edges
        tgt[ties] = yhat[ties]

    yl = yhat.double().clone().requires_grad_()
    per_node = torch.stack([
        loss_cls()(yl[l * B:(l + 1) * B], tgt.double()[l * B:(l + 1) * B])
        for l in range(Lr)
    ])
    (loss_scale * per_node.sum()).backward()
    ref_dy, ref_loss = yl.grad, per_node.detach()
    if kind == "l1":
        assert (ref_dy[ties] == 0).all()  # torch's sign(0) is 0

    dev = _dev()
    dbuf, dY = _guarded(Lr * B, dtype)
    lbuf, loss = _guarded(Lr, dtype, fill=0.0)  # the kernel adds into it
    ext.regression_bwd(yhat.to(dev), tgt.to(dev), dY, loss, B,
                       loss_scale, mode)
    tag = f"regression_bwd {kind} {dtype}"
    print(f"{tag} dY max|err| = "
          f"{(dY.cpu().double() - ref_dy).abs().max().item():.3e} "
          f"loss max|err| = "
          f"{(loss.cpu().double() - ref_loss).abs().max().item():.3e}")
    torch.testing.assert_close(dY.cpu(), ref_dy.to(dtype), **TOL[dtype])
    torch.testing.assert_close(loss.cpu(), ref_loss.to(dtype),
                               **TOL[dtype])
    if kind == "l1":
        assert (dY.cpu()[ties] == 0).all()
    _assert_guards(dbuf, tag + " dY")
    _assert_guards(lbuf, tag + " loss")

    # loss = None: the same gradient, and no loss accumulation
    dbuf2, dY2 = _guarded(Lr * B, dtype)
    ext.regression_bwd(yhat.to(dev), tgt.to(dev), dY2, None, B,
                       loss_scale, mode)
    torch.testing.assert_close(dY2, dY, rtol=0, atol=0)
    _assert_guards(dbuf2, tag + " dY (no loss)")
