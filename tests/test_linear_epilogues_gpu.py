"""Activation epilogues of the stacked linear kernels vs fp64 torch.

linear_bwd_dx with the below layer's activation backward fused into its
epilogue (VALU kernel, and the three epilogues of the MFMA kernel: relu
fast path, encode-recompute fast path, generic guarded), linear_fwd on
the MFMA kernel with every activation with and without the Z stash, the
I == 1 small-K forward routes, and act_grad for every activation.

Every input is drawn on the CPU from a seeded generator, rounded to the
test dtype, and the reference is plain fp64 torch (autograd where a
gradient is checked) on those rounded inputs, so the two preconditions
of the recompute cases (distance of scale*z from the sin_relu kink) are
facts about the seed, not about the device. The layer sits at a nonzero
even offset of an even-length parameter row between sentinel pads, the
outputs sit between sentinel guards, and nothing but the output range
may change.

Magnitudes: dZ and x are standard normal, W is normal with std
1/sqrt(contraction length) (dx) resp. 2/sqrt(I) (fwd), so |dX| stays
below ~6 and |z| below ~12. A sin_relu argument scale*z then stays
below ~25 rad, where an fp32 product and sin/cos carry at most about
25 * 2^-23 = 3e-6 of absolute error; times scale (1.75) and |dX| <= 6
that is 3e-5 in the very worst element and about 1e-6 typically, inside
TOL's fp32 bound (2e-5 + 2e-4 |ref|). SCALE = 1.75 is exact in fp32, so
no rounding of the scale itself separates kernel and reference.
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

ACT = {"none": 0, "relu": 1, "sin_relu": 2, "sigmoid": 3, "tanh": 4}
SCALE = 1.75
SENTINEL = 1000.0
GUARD = 64          # sentinel elements before and after every output
SEED_DX = 31
SEED_FWD = 32
SEED_ACT = 33
L = 2

# fp32 recompute: elements this close to the kink may be left out, and
# at most this share of them
KINK_SKIP = 1e-4
KINK_SHARE_MAX = 1e-3
KINK_MIN_F64 = 1e-9


@pytest.fixture(scope="module")
def ext():
    from nn_distributed_training_amd.ops import get_ext

    return get_ext()


def _dev():
    return torch.device("cuda")


def _act_ref(name, z):
    if name == "relu":
        return torch.relu(z)
    if name == "sin_relu":
        return torch.relu(torch.sin(SCALE * z))
    if name == "sigmoid":
        return torch.sigmoid(z)
    if name == "tanh":
        return torch.tanh(z)
    return z


def _guarded(numel, dtype):
    """A sentinel-filled device buffer and the contiguous view of its
    middle `numel` elements (even guard: 16-byte alignment is kept)."""
    buf = torch.full((GUARD + numel + GUARD,), SENTINEL, dtype=dtype,
                     device=_dev())
    return buf, buf[GUARD:GUARD + numel]


def _assert_guards(buf, what):
    assert (buf[:GUARD] == SENTINEL).all(), f"{what}: wrote below range"
    assert (buf[-GUARD:] == SENTINEL).all(), f"{what}: wrote above range"


def _away_from_kink(shape, gen):
    """fp64 z with SCALE*z = (k + u)*pi, k in [-4, 3], u in [.05, .95]:
    both signs of sin, cos over its whole range, never near the kink."""
    k = torch.randint(-4, 4, shape, generator=gen).double()
    u = 0.05 + 0.9 * torch.rand(shape, generator=gen, dtype=torch.float64)
    return (k + u) * math.pi / SCALE


def _report(tag, got, ref):
    err = (got.double() - ref).abs().max().item()
    print(f"{tag} max|err| = {err:.3e}")


# ---------------------------------------------------------------------
# 1. dX with the fused below-activation vs autograd

DX_SHAPES = [
    (40, 24, 16),     # VALU linear_bwd_dx_k (M < 128)
    (150, 70, 40),    # mfma_dx_k: ragged m- and i-edge tiles (generic
                      # epilogue) around two full tiles (m0 = 0, 64 at
                      # i0 = 0); guarded 8-wide tail stage
    (128, 64, 8),     # every tile full; O = 8 < FK: guarded load stage
                      # feeding a full-tile epilogue
    (150, 134, 40),   # full and ragged blocks in one launch, m and i
]
DX_VARIANTS = [
    "none", "relu", "sigmoid", "tanh", "sin_relu_stored",
    "sin_relu_ib1", "sin_relu_ib2", "sin_relu_ib3", "sin_relu_ib4",
]


def dx_case(dtype, M, I, O, variant):
    """Inputs (CPU, test dtype), the layout and the fp64 reference of
    one dX case; `kink` is |sin(SCALE*z)| of the recomputed z, else
    None. Device-free, so the seed's preconditions can be checked
    anywhere."""
    gen = torch.Generator().manual_seed(SEED_DX)
    recompute = variant.startswith("sin_relu_ib")
    Ib = int(variant[-1]) if recompute else 0
    act = variant if variant in ("none", "relu", "sigmoid", "tanh") \
        else "sin_relu"

    # row: [pad | Wb [I, Ib] | bb [I] | pad | W [O, I] | pad]
    pad_lo, pad_mid, pad_hi = 6, 10, 8
    wb_off = pad_lo
    bb_off = wb_off + I * Ib
    w_off = bb_off + I + pad_mid
    n = w_off + O * I + pad_hi
    assert w_off % 2 == 0 and w_off > 0 and n % 2 == 0
    theta = torch.full((L, n), SENTINEL, dtype=torch.float64)
    W = torch.randn(L, O, I, generator=gen, dtype=torch.float64) \
        / math.sqrt(O)
    theta[:, w_off:w_off + O * I] = W.reshape(L, -1)
    dZ = torch.randn(L, M, O, generator=gen, dtype=torch.float64)

    Xb2 = None
    if recompute:
        Wb = torch.randn(L, I, Ib, generator=gen, dtype=torch.float64)
        bb = torch.randn(L, I, generator=gen, dtype=torch.float64)
        Xb2 = torch.randn(L, M, Ib, generator=gen, dtype=torch.float64)
        theta[:, wb_off:bb_off] = Wb.reshape(L, -1)
        theta[:, bb_off:bb_off + I] = bb
    elif act == "sin_relu":
        zb = _away_from_kink((L, M, I), gen)
    else:
        zb = torch.randn(L, M, I, generator=gen, dtype=torch.float64)

    # round to the test dtype; the reference sees the rounded values
    theta = theta.to(dtype)
    dZ = dZ.to(dtype)
    th64 = theta.double()
    if recompute:
        Xb2 = Xb2.to(dtype)
        Wb64 = th64[:, wb_off:bb_off].reshape(L, I, Ib)
        bb64 = th64[:, bb_off:bb_off + I]
        zb64 = torch.einsum("lmj,lij->lmi", Xb2.double(), Wb64) \
            + bb64[:, None, :]
        zb_dt = None
    else:
        zb_dt = zb.to(dtype)
        zb64 = zb_dt.double()

    zleaf = zb64.clone().requires_grad_()
    yb64 = _act_ref(act, zleaf)
    W64 = th64[:, w_off:w_off + O * I].reshape(L, O, I)
    torch.einsum("lmi,loi->lmo", yb64, W64).backward(dZ.double())
    ref = zleaf.grad.reshape(L * M, I)

    kink = torch.sin(SCALE * zb64).abs().reshape(L * M, I) \
        if recompute else None
    return dict(
        theta=theta, dZ=dZ.reshape(L * M, O), Xb2=Xb2, Ib=Ib,
        Yb=yb64.detach().to(dtype).reshape(L * M, I),
        Zb=None if zb_dt is None else zb_dt.reshape(L * M, I),
        act=act, recompute=recompute, w_off=w_off, wb_off=wb_off,
        bb_off=bb_off, ref=ref, kink=kink,
    )


def dx_kink_stats(case):
    """(min |sin(SCALE*z)|, share of elements below KINK_SKIP)."""
    k = case["kink"]
    return k.min().item(), (k < KINK_SKIP).double().mean().item()


@requires_gpu
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("variant", DX_VARIANTS)
@pytest.mark.parametrize("M,I,O", DX_SHAPES)
def test_linear_bwd_dx_fused_act_matches_autograd(ext, dtype, M, I, O,
                                                  variant):
    """dX = (dZ @ W) * act'(z_below) in one launch, for every below
    activation and both sources of z_below (stored Zb; recomputed from
    the below layer's Ib-wide input), vs autograd through
    yb = act(zb); yb @ W^T."""
    c = dx_case(dtype, M, I, O, variant)
    dev = _dev()
    theta = c["theta"].to(dev)
    theta0 = theta.clone()
    act = c["act"]
    buf, flat = _guarded(L * M * I, dtype)
    dX = flat.view(L * M, I)

    Yb = None if act == "none" else c["Yb"].to(dev)
    Zb = None if c["Zb"] is None or act != "sin_relu" \
        else c["Zb"].to(dev)
    if c["recompute"]:
        ext.linear_bwd_dx(c["dZ"].to(dev), theta, dX, Yb, None,
                          ACT[act], SCALE, c["w_off"], M, I, O,
                          c["Xb2"].reshape(L * M, c["Ib"]).to(dev),
                          c["wb_off"], c["bb_off"], c["Ib"])
    else:
        ext.linear_bwd_dx(c["dZ"].to(dev), theta, dX, Yb, Zb, ACT[act],
                          SCALE, c["w_off"], M, I, O, None, 0, 0, 0)

    got = dX.cpu()
    ref = c["ref"]
    tag = f"dx {M}x{I}x{O} {variant} {dtype}"
    if c["recompute"]:
        kmin, share = dx_kink_stats(c)
        print(f"{tag} min|sin| = {kmin:.3e} skip share = {share:.2e}")
        if dtype == torch.float64:
            assert kmin > KINK_MIN_F64
        else:
            assert share <= KINK_SHARE_MAX
            skip = c["kink"] < KINK_SKIP
            got = torch.where(skip, ref.to(dtype), got)
    _report(tag, got, ref)
    torch.testing.assert_close(got, ref.to(dtype), **TOL[dtype])
    _assert_guards(buf, tag)
    assert torch.equal(theta, theta0), f"{tag}: parameters changed"


# ---------------------------------------------------------------------
# 2. forward: every activation, with and without the Z stash

FWD_ACTS = ["none", "relu", "sin_relu", "sigmoid", "tanh"]
FWD_SHAPES = [
    (128, 32, 64),    # all tiles full, one full stage
    (128, 8, 16),     # the MFMA dispatch minimum
    (150, 70, 40),    # all tiles ragged
    (150, 34, 70),    # mixed tiles and a 2-wide K tail
]
SMALLK_SHAPES = [
    (1024, 1, 64),    # encode_fwd_k<T, 1>
    (1024, 1, 10),    # linear_fwd_smallk_k at I = 1
]


def _fwd_check(ext, dtype, M, I, O, act, with_z):
    gen = torch.Generator().manual_seed(SEED_FWD)
    pad_lo, pad_mid, pad_hi = 6, 4, 8 + (O * I + O) % 2
    w_off = pad_lo
    b_off = w_off + O * I + pad_mid
    n = b_off + O + pad_hi
    assert w_off % 2 == 0 and n % 2 == 0
    theta = torch.full((L, n), SENTINEL, dtype=torch.float64)
    theta[:, w_off:w_off + O * I] = torch.randn(
        L, O * I, generator=gen, dtype=torch.float64) * 2 / math.sqrt(I)
    theta[:, b_off:b_off + O] = torch.randn(
        L, O, generator=gen, dtype=torch.float64)
    theta = theta.to(dtype)
    X = torch.randn(L, M, I, generator=gen, dtype=torch.float64).to(dtype)

    th64 = theta.double()
    z_ref = torch.einsum(
        "lmi,loi->lmo", X.double(),
        th64[:, w_off:w_off + O * I].reshape(L, O, I),
    ) + th64[:, None, b_off:b_off + O]
    z_ref = z_ref.reshape(L * M, O)
    y_ref = _act_ref(act, z_ref)

    dev = _dev()
    theta_d = theta.to(dev)
    theta0 = theta_d.clone()
    ybuf, yflat = _guarded(L * M * O, dtype)
    Y = yflat.view(L * M, O)
    zbuf, Z = None, None
    if with_z:
        zbuf, zflat = _guarded(L * M * O, dtype)
        Z = zflat.view(L * M, O)
    ext.linear_fwd(X.reshape(L * M, I).to(dev), theta_d, Y, Z, w_off,
                   b_off, M, I, O, ACT[act], SCALE)

    tag = f"fwd {M}x{I}x{O} {act} z={int(with_z)} {dtype}"
    _report(tag + " Y", Y.cpu(), y_ref)
    torch.testing.assert_close(Y.cpu(), y_ref.to(dtype), **TOL[dtype])
    _assert_guards(ybuf, tag + " Y")
    if with_z:
        _report(tag + " Z", Z.cpu(), z_ref)
        torch.testing.assert_close(Z.cpu(), z_ref.to(dtype),
                                   **TOL[dtype])
        _assert_guards(zbuf, tag + " Z")
    assert torch.equal(theta_d, theta0), f"{tag}: parameters changed"


@requires_gpu
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("with_z", [False, True])
@pytest.mark.parametrize("act", FWD_ACTS)
@pytest.mark.parametrize("M,I,O", FWD_SHAPES)
def test_mfma_fwd_activations_and_z_stash(ext, dtype, M, I, O, act,
                                          with_z):
    """mfma_fwd_k: Y = act(X @ W^T + b) and the stashed Z. A non-null Z
    sends even full tiles through the guarded epilogue."""
    _fwd_check(ext, dtype, M, I, O, act, with_z)


@requires_gpu
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("with_z", [False, True])
@pytest.mark.parametrize("act", ["sin_relu", "sigmoid"])
@pytest.mark.parametrize("M,I,O", SMALLK_SHAPES)
def test_linear_fwd_smallk_in_dim_one(ext, dtype, M, I, O, act, with_z):
    """The two small-K forward kernels at I == 1."""
    _fwd_check(ext, dtype, M, I, O, act, with_z)


# ---------------------------------------------------------------------
# 3. act_grad for every activation vs autograd

@requires_gpu
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("act", FWD_ACTS)
def test_act_grad_every_activation(ext, dtype, act):
    """dZ = dY * act'(z): from Y alone, except sin_relu which reads Z."""
    gen = torch.Generator().manual_seed(SEED_ACT)
    rows, cols = L * 37, 9          # 666 elements: 2 blocks + a tail
    assert (rows * cols) % 256 != 0
    if act == "sin_relu":
        z = _away_from_kink((rows, cols), gen).to(dtype)
    else:
        z = torch.randn(rows, cols, generator=gen,
                        dtype=torch.float64).to(dtype)
    dY = torch.randn(rows, cols, generator=gen,
                     dtype=torch.float64).to(dtype)
    zleaf = z.double().clone().requires_grad_()
    y64 = _act_ref(act, zleaf)
    y64.backward(dY.double())
    ref = zleaf.grad

    dev = _dev()
    buf, flat = _guarded(rows * cols, dtype)
    dZ = flat.view(rows, cols)
    ext.act_grad(dY.to(dev), y64.detach().to(dtype).to(dev),
                 z.to(dev) if act == "sin_relu" else None, dZ,
                 ACT[act], SCALE)
    tag = f"act_grad {act} {dtype}"
    _report(tag, dZ.cpu(), ref)
    torch.testing.assert_close(dZ.cpu(), ref.to(dtype), **TOL[dtype])
    _assert_guards(buf, tag)
