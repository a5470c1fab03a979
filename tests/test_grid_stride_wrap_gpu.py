"""Second trip of the elementwise grid-stride loops vs fp64 torch.

Every elementwise and loss kernel launches at most 4096 blocks of 256
threads and strides over the rest. At L = 5, n = 262147 the stack has
1,310,735 elements: 262,159 of them are reached only on a thread's
second trip, and the boundary between rows 3 and 4 (element 1,048,588)
lies inside that wrapped part, so the `t / n` row split runs there too.
The references are the ones tests/test_ops_gpu.py uses at its small
shapes, computed in fp64 from the dtype-rounded inputs.
"""

import pytest
import torch

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(
    not torch.cuda.is_available(), reason="needs MI355X"
)

TOL = {torch.float64: dict(rtol=1e-10, atol=1e-10),
       torch.float32: dict(rtol=2e-4, atol=2e-5)}

L, N = 5, 262147
CAP = 4096 * 256
SEED = 51
DTYPES = [torch.float64, torch.float32]

assert L * N - CAP == 262159 and 4 * N > CAP  # the wrap holds a row edge


@pytest.fixture(scope="module")
def ext():
    from nn_distributed_training_amd.ops import get_ext

    return get_ext()


def _dev():
    return torch.device("cuda")


def _randn(*shape, dtype):
    return torch.randn(*shape, dtype=torch.float64,
                       device=_dev()).to(dtype)


def _close(tag, got, ref, dtype):
    """Compare with TOL, reporting the whole tensor and its wrapped
    tail (flat elements >= CAP) separately."""
    err = (got.double() - ref).abs().reshape(-1)
    tail = err[CAP:].max().item() if err.numel() > CAP else float("nan")
    print(f"{tag} {dtype} max|err| = {err.max().item():.3e} "
          f"(wrapped part {tail:.3e})")
    torch.testing.assert_close(got, ref.to(dtype), **TOL[dtype])


def _csr():
    """Rows 0..4 local, 5..6 remote. Node 2 has no neighbour, node 4
    (the row the wrap crosses into) reads a remote and a local row."""
    nbrs = [[1, 5], [0, 2, 6], [], [4, 6], [3, 5]]
    offs, idx = [0], []
    for nb in nbrs:
        idx += nb
        offs.append(len(idx))
    dev = _dev()
    return (nbrs, torch.tensor(offs, dtype=torch.int32, device=dev),
            torch.tensor(idx, dtype=torch.int32, device=dev))


@requires_gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_wrap_dinno_dual_threg(ext, dtype):
    torch.manual_seed(SEED)
    nbrs, offs, idx = _csr()
    local = _randn(L, N, dtype=dtype)
    remote = _randn(2, N, dtype=dtype)
    duals = _randn(L, N, dtype=dtype)
    duals0 = duals.double().clone()
    s = torch.empty_like(duals)
    rho = 0.37
    ext.dinno_dual_threg(local, remote, offs, idx, duals, s, rho)

    table = torch.cat([local, remote]).double()
    S = torch.stack([
        sum((table[j] for j in nb), torch.zeros_like(table[0]))
        for nb in nbrs
    ])
    deg = torch.tensor([len(nb) for nb in nbrs], dtype=torch.float64,
                       device=_dev())[:, None]
    _close("wrap dual", duals, duals0 + rho * (deg * table[:L] - S),
           dtype)
    _close("wrap s", s, (deg * table[:L] + S) / 2, dtype)


@requires_gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_wrap_mix_rows(ext, dtype):
    torch.manual_seed(SEED + 1)
    nbrs, offs, idx = _csr()
    local = _randn(L, N, dtype=dtype)
    remote = _randn(2, N, dtype=dtype)
    w = _randn(idx.numel(), dtype=dtype)
    out = torch.empty_like(local)
    ext.mix_rows(local, remote, offs, idx, w, out)

    table = torch.cat([local, remote]).double()
    ref = torch.zeros(L, N, dtype=torch.float64, device=_dev())
    k = 0
    for l, nb in enumerate(nbrs):
        for j in nb:
            ref[l] += w[k].double() * table[j]
            k += 1
    _close("wrap mix_rows", out, ref, dtype)


@requires_gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_wrap_dsgt_mix_and_y_update(ext, dtype):
    torch.manual_seed(SEED + 2)
    nbrs, offs, idx = _csr()
    p_loc = _randn(L, N, dtype=dtype)
    y_loc = _randn(L, N, dtype=dtype)
    rem2 = _randn(2, 2 * N, dtype=dtype)   # bundles [p | y]
    w = _randn(idx.numel(), dtype=dtype)
    alpha = 0.05
    p_out = torch.empty_like(p_loc)
    y_mix = torch.empty_like(p_loc)
    ext.dsgt_mix(p_loc, y_loc, rem2, offs, idx, w, p_out, y_mix, alpha)

    ptab = torch.cat([p_loc, rem2[:, :N]]).double()
    ytab = torch.cat([y_loc, rem2[:, N:]]).double()
    accp = torch.zeros(L, N, dtype=torch.float64, device=_dev())
    accy = torch.zeros_like(accp)
    k = 0
    for l, nb in enumerate(nbrs):
        for j in nb:
            accp[l] += w[k].double() * ptab[j]
            accy[l] += w[k].double() * ytab[j]
            k += 1
    _close("wrap dsgt p_out", p_out, accp - alpha * accy, dtype)
    _close("wrap dsgt y_mix", y_mix, accy, dtype)

    g_new = _randn(L, N, dtype=dtype)
    g_old = _randn(L, N, dtype=dtype)
    g_old0 = g_old.double().clone()
    y = torch.empty_like(g_new)
    ext.dsgt_y_update(y_mix, g_new, g_old, y)
    _close("wrap dsgt y", y, y_mix.double() + g_new.double() - g_old0,
           dtype)
    assert torch.equal(g_old, g_new)


@requires_gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nparts", [1, 3])
def test_wrap_fused_step_adam(ext, dtype, nparts):
    """Two DiNNO primal Adam steps (the second reads the moments) with
    the gradient in `nparts` slabs and zero_grad=True, vs torch's Adam
    fed the analytic primal gradient.

    eps = 1e-3, not Adam's 1e-8: the update lr*m/(sqrt(v)+eps) changes
    by up to lr/eps per unit of gradient error, and among 1.3 million
    gradients some are far smaller than their own fp32 rounding error
    (~1e-7); lr/eps = 10 keeps that below TOL's atol, 1e6 would not."""
    torch.manual_seed(SEED + 3)
    dev = _dev()
    theta = _randn(L, N, dtype=dtype)
    duals = _randn(L, N, dtype=dtype)
    s = _randn(L, N, dtype=dtype)
    deg_list = [2, 3, 0, 2, 2]       # node 2 is isolated: stays frozen
    deg = torch.tensor(deg_list, dtype=torch.int32, device=dev)
    degf = deg.double()[:, None]
    gparts = _randn(L, nparts, N, dtype=dtype)
    grad = gparts.clone()
    m = torch.zeros_like(theta)
    v = torch.zeros_like(theta)
    rho, lr, eps = 0.21, 0.01, 1e-3

    p = theta.double().clone().requires_grad_()
    opt = torch.optim.Adam([p], lr, eps=eps)
    theta0 = theta.double().clone()
    for step in (1, 2):
        if step == 2:
            grad.copy_(gparts)
        ext.fused_step(theta, grad, duals, s, deg, m, v, rho, lr, 0.9,
                       0.999, eps, 0.0, step, 0, step == 1, nparts, True)
        assert not grad.any(), "zero_grad left gradient behind"
        with torch.no_grad():
            g = gparts.double().sum(dim=1) + duals.double() \
                + 2 * rho * (degf * p - s.double())
            g[2] = 0
        p.grad = g
        opt.step()
        with torch.no_grad():
            p[2] = theta0[2]  # an isolated node takes no step at all
        _close(f"wrap fused_step nparts={nparts} step {step}", theta,
               p.detach(), dtype)
    assert torch.equal(theta[2].double(), theta0[2])


@requires_gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("zero_grad", [False, True])
def test_wrap_axpy(ext, dtype, zero_grad):
    torch.manual_seed(SEED + 4)
    x = _randn(L, N, dtype=dtype)
    g = _randn(L, N, dtype=dtype)
    x0, g0 = x.double().clone(), g.clone()
    ext.axpy(x, g, -0.3, zero_grad)
    _close(f"wrap axpy zero_grad={zero_grad}", x, x0 - 0.3 * g0.double(),
           dtype)
    if zero_grad:
        assert not g.any()
    else:
        assert torch.equal(g, g0)


@requires_gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_wrap_reduce_parts(ext, dtype):
    torch.manual_seed(SEED + 5)
    parts = _randn(L, 3, N, dtype=dtype)
    out = torch.empty(L, N, dtype=dtype, device=_dev())
    ext.reduce_parts(parts, out, 3)
    _close("wrap reduce_parts", out, parts.double().sum(dim=1), dtype)


@requires_gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_wrap_act_grad_relu(ext, dtype):
    torch.manual_seed(SEED + 6)
    Y = torch.relu(_randn(L, N, dtype=dtype))
    dY = _randn(L, N, dtype=dtype)
    dZ = torch.empty_like(dY)
    ext.act_grad(dY, Y, None, dZ, 1, 1.0)
    _close("wrap act_grad relu", dZ,
           torch.where(Y > 0, dY, torch.zeros_like(dY)).double(), dtype)


@requires_gpu
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind,mode", [("mse", 0), ("l1", 1)])
def test_wrap_regression_bwd(ext, dtype, kind, mode):
    """B = n: one node per row. fp64 also checks the per-node loss;
    fp32 runs the loss = None form (262147 unordered fp32 atomic adds
    per node have no stable reference)."""
    torch.manual_seed(SEED + 7)
    yhat = _randn(L * N, dtype=dtype)
    tgt = _randn(L * N, dtype=dtype)
    loss_scale = 0.7
    d = (yhat.double() - tgt.double()).reshape(L, N)
    if kind == "mse":
        ref_dy, ref_loss = 2 * d * loss_scale / N, (d * d).mean(dim=1)
    else:
        ref_dy, ref_loss = torch.sign(d) * loss_scale / N, \
            d.abs().mean(dim=1)
    dY = torch.empty_like(yhat)
    loss = None
    if dtype == torch.float64:
        loss = torch.zeros(L, dtype=dtype, device=_dev())
    ext.regression_bwd(yhat, tgt, dY, loss, N, loss_scale, mode)
    # |dY| ~ 1e-6 here, under TOL's atol, where the comparison would
    # pass whatever the kernel wrote: compare N * dY, of order 1 (the
    # rescale costs one more rounding, 1 ulp)
    _close(f"wrap regression_bwd {kind} N*dY", dY.reshape(L, N) * N,
           ref_dy * N, dtype)
    if loss is not None:
        _close(f"wrap regression_bwd {kind} loss", loss, ref_loss, dtype)


@requires_gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_gather_targets_floating(ext, dtype):
    """gather_targets on floating densities (the small shape of
    test_gather_batch, which gathers long labels only)."""
    torch.manual_seed(9)
    Lg, maxlen, B, S = 3, 50, 8, 40
    dev = _dev()
    Yt = torch.randn(Lg, maxlen, dtype=dtype, device=dev)
    stream = torch.randint(0, maxlen, (Lg, S), device=dev)
    view = stream[:, 5:5 + B]
    ar = torch.arange(Lg, device=dev).unsqueeze(1)
    ref = Yt[ar, view].reshape(-1)
    yb = torch.full((Lg * B,), -7.0, dtype=dtype, device=dev)
    ext.gather_targets(Yt, view.contiguous(), yb, B, 0)
    torch.testing.assert_close(yb, ref, rtol=0, atol=0)
    yb2 = torch.full((Lg * B,), -7.0, dtype=dtype, device=dev)
    ext.gather_targets(Yt, stream, yb2, S, 5)
    torch.testing.assert_close(yb2, ref, rtol=0, atol=0)
