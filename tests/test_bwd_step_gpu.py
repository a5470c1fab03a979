"""The DiNNO primal step folded into the backward launch
(ext.dw_dx0_conv_bwd_step_idx / ext.mnist_fwd_bwd_step, fused_mnist.hip
dw_dx0_conv_bwd_k with STEP on).

The reference is always the sequence the launch replaces, on clones of
one state: ext.dw_dx0_conv_bwd_idx, then ext.fused_step_dual (the step
that carries the dual ascent) or ext.fused_step (the plain one).

dz1, theta's W1 slice and the images are small integers in [-2, 2] (x0
in [0, 2]), so dX0 and every atomically accumulated conv sum are exact
in fp32 and fp64 in any order (largest sum here: 128 * 144 items of at
most 64 * 4 * 2 = 512 < 2^24): all comparisons are bit for bit. Only the
driver-level test has a tolerance, because the fc block's fc2 atomics
see real-valued data: it allows 10x the difference two old-path runs
show between themselves, as tests/test_step_dual_gpu.py does.
"""

import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(
    not torch.cuda.is_available(), reason="needs MI355X"
)

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
RHO, LR, B1, B2, EPS = 0.37, 0.005, 0.9, 0.999, 1e-8
OFF = 3          # batch offset into the index stream
SENTINEL = 7.0   # what the fc1 grad slice holds before the new launch

# (L, M, IMG, K, F, H, C): the smallest shape the dispatch takes is
# IMG 12, K 5 (a 4 x 4 pooled map: one 16-column strip per filter);
# F = 2 gives every node two conv blocks, so a ticket is drawn twice.
BASE = (3, 16, 12, 5, 2, 16, 10)


@pytest.fixture(scope="module")
def ext():
    from nn_distributed_training_amd.ops import get_ext

    return get_ext()


def _csr(nbrs, dev):
    offs, idx = [0], []
    for row in nbrs:
        idx += row
        offs.append(len(idx))
    mk = lambda x: torch.tensor(x, dtype=torch.int32, device=dev)
    return mk(offs), mk(idx), mk([len(r) for r in nbrs])


def _ring(L):
    return [[(i - 1) % L, (i + 1) % L] for i in range(L)]


class Case:
    """Inputs of one backward + step at a shape, and the layout."""

    def __init__(self, shape, dtype, seed=0):
        L, M, IMG, K, F, H, C = shape
        self.shape, self.dtype = shape, dtype
        P = (IMG - (K - 1)) // 2
        I = F * P * P
        self.I = I
        self.cw, self.cb = 0, F * K * K
        self.w1 = self.cb + F
        self.b1 = self.w1 + H * I
        self.w2 = self.b1 + H
        self.b2 = self.w2 + C * H
        self.n = n = self.b2 + C
        dev = torch.device("cuda")
        g = torch.Generator(device="cuda").manual_seed(100 + seed)
        rnd = lambda *sh: torch.randn(
            *sh, dtype=dtype, device=dev, generator=g)
        ints = lambda lo, hi, *sh: torch.randint(
            lo, hi + 1, sh, device=dev, generator=g).to(dtype)
        maxlen, self.stride = M + 9, M + 7
        self.X_all = ints(-2, 2, L, maxlen, IMG * IMG)
        self.src_idx = torch.randint(
            0, maxlen, (L, self.stride), device=dev, generator=g)
        self.pidx = torch.randint(
            0, 4, (L * M, I), device=dev, generator=g).to(torch.uint8)
        self.x0 = ints(0, 2, L * M, I)
        self.dz1 = ints(-2, 2, L * M, H)
        theta = rnd(L, n)
        theta[:, self.w1:self.b1] = ints(-2, 2, L, H * I)
        # what the fc block leaves: fc2's sums complete, conv's zero
        grad = torch.zeros(L, n, dtype=dtype, device=dev)
        grad[:, self.w2:] = rnd(L, n - self.w2)
        self.state = dict(
            theta=theta, grad=grad, duals=rnd(L, n), s=rnd(L, n),
            m=rnd(L, n) * 0.1, v=rnd(L, n).abs() * 0.01)
        self.rnd = rnd

    def small(self, t):
        """The atomically accumulated slices of a [L, n] tensor."""
        return torch.cat([t[:, :self.w1], t[:, self.w2:]], dim=1)

    def bwd_args(self, theta, grad):
        L, M, IMG, K, F, H, C = self.shape
        return (self.dz1, self.x0, theta, self.pidx, self.X_all,
                self.src_idx, self.stride, OFF, grad, self.w1, self.b1,
                M, self.I, H, self.cw, self.cb, F, K, IMG)


def _fused_for(ext, shape, dtype):
    L, M, IMG, K, F, H, C = shape
    P = (IMG - (K - 1)) // 2
    es = 8 if dtype == torch.float64 else 4
    return ext.bwd_step_fused_for(L, M, F * P * P, H, F, K, IMG, es, 1)


def _reference(ext, case, st, remote, csr, dual, mode, wd, first, step_t):
    """Today's two launches on clones; returns the state after them."""
    offs, idx, deg = csr
    old = {k: t.clone() for k, t in st.items()}
    mv = (None, None) if mode == 2 else (old["m"], old["v"])
    ext.dw_dx0_conv_bwd_idx(*case.bwd_args(old["theta"], old["grad"]))
    if dual:
        ext.fused_step_dual(
            old["theta"], old["grad"], remote, offs, idx, deg,
            old["duals"], old["s"], *mv, RHO, LR, B1, B2, EPS, wd, step_t,
            mode, first, 1, True)
    else:
        ext.fused_step(
            old["theta"], old["grad"], old["duals"], old["s"], deg, *mv,
            RHO, LR, B1, B2, EPS, wd, step_t, mode, first, 1, True)
    return old


def _new(ext, case, st, theta_out, remote, csr, dual, mode, wd, first,
         step_t):
    """The new entry on clones; grad's fc1 slice starts as SENTINEL.
    Returns (state after, theta_out, whether the launch was fused)."""
    L, M, IMG, K, F, H, C = case.shape
    offs, idx, deg = csr
    new = {k: t.clone() for k, t in st.items()}
    new["grad"][:, case.w1:case.w2] = SENTINEL
    mv = (None, None) if mode == 2 else (new["m"], new["v"])
    fused = ext.dw_dx0_conv_bwd_step_idx(
        *case.bwd_args(new["theta"], new["grad"])[:3], theta_out,
        *case.bwd_args(new["theta"], new["grad"])[3:], case.w2, case.b2,
        C, remote, offs, idx, deg, new["duals"], new["s"], *mv, RHO, LR,
        B1, B2, EPS, wd, step_t, mode, first, dual)
    return new, fused


def _check(ext, case, nbrs, dual, mode=0, wd=0.0, first=True, remote=None,
           st=None):
    """One launch against the reference, everything bit for bit.
    Returns (state before, state after, theta_out)."""
    dev = torch.device("cuda")
    assert _fused_for(ext, case.shape, case.dtype)
    st = st if st is not None else case.state
    csr = _csr(nbrs, dev)
    step_t = 1 if first else 3
    old = _reference(ext, case, st, remote, csr, dual, mode, wd, first,
                     step_t)
    theta_out = torch.full_like(st["theta"], float("nan"))
    new, fused = _new(ext, case, st, theta_out, remote, csr, dual, mode,
                      wd, first, step_t)
    torch.cuda.synchronize()
    assert fused
    # theta_in is only read
    assert torch.equal(new["theta"], st["theta"])
    assert torch.isfinite(theta_out).all()
    assert torch.equal(theta_out, old["theta"])
    for k in ("duals", "s", "m", "v"):
        assert torch.equal(new[k], old[k]), k
    assert (case.small(new["grad"]) == 0).all()
    assert (new["grad"][:, case.w1:case.w2] == SENTINEL).all()
    return st, new, theta_out


# --------------------------------------------------------------- tests --
@requires_gpu
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("dual", [True, False])
def test_equality(ext, dtype, dual):
    """Both variants, first step or not, Adam, AdamW (with decay), SGD,
    and Adam with L2 decay."""
    case = Case(BASE, dtype)
    for first in (True, False):
        for mode, wd in ((0, 0.0), (1, 0.01), (2, 0.0), (0, 0.01)):
            st, new, theta_out = _check(
                ext, case, _ring(BASE[0]), dual, mode=mode, wd=wd,
                first=first)
            assert not torch.equal(theta_out, st["theta"])
            # the plain step reads duals and s, it does not write them
            assert torch.equal(new["duals"], st["duals"]) == (not dual)
            assert torch.equal(new["s"], st["s"]) == (not dual)
            if mode == 2:
                assert torch.equal(new["m"], st["m"])


@requires_gpu
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_hazard_complete_graph(ext, dtype):
    """Every node reads every other node's round-start theta while the
    stepped theta is being written: theta_in must come out untouched and
    theta_out, NaN before, finite and equal to the reference (_check
    asserts all three)."""
    L = 8
    shape = (L,) + BASE[1:]
    nbrs = [[j for j in range(L) if j != i] for i in range(L)]
    _check(ext, Case(shape, dtype), nbrs, True, first=False)


@requires_gpu
@pytest.mark.parametrize("dual", [True, False])
def test_isolated_node(ext, dual):
    """Degrees 1, 2, 1, 0: the isolated node's theta_out row is its
    theta_in row, and its moments are frozen."""
    shape = (4,) + BASE[1:]
    st, new, theta_out = _check(
        ext, Case(shape, torch.float64), [[1], [0, 2], [1], []], dual,
        first=False)
    assert torch.equal(theta_out[3], st["theta"][3])
    for k in ("m", "v", "duals"):
        assert torch.equal(new[k][3], st[k][3]), k
    for k in ("m", "v"):
        assert not torch.equal(new[k][:3], st[k][:3]), k
    if dual:
        assert (new["s"][3] == 0).all()


@requires_gpu
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_remote_rows(ext, dtype):
    """Two received rows (table rows 3 and 4) among the neighbours, in
    an order that is not ascending."""
    case = Case(BASE, dtype)
    _check(ext, case, [[3, 1], [0, 2], [4, 1, 0]], True,
           remote=case.rnd(2, case.n))


@requires_gpu
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_ticket_reuse(ext, dtype):
    """A -> B with the dual ascent, then B -> A plain, with no workspace
    reset in between; then a launch at another L. The tickets must come
    back to zero after every launch for the next one to find its last
    block."""
    case = Case(BASE, dtype)
    st, new, theta_b = _check(ext, case, _ring(3), True)
    st2 = dict(new, theta=theta_b, grad=case.state["grad"])
    _check(ext, case, _ring(3), False, first=False, st=st2)
    _check(ext, Case((5,) + BASE[1:], dtype, seed=1), _ring(5), True)
    _check(ext, Case((2,) + BASE[1:], dtype, seed=2), _ring(2), False,
           first=False)


@requires_gpu
@pytest.mark.parametrize("dual", [True, False])
def test_two_conv_blocks_per_strip(ext, dual):
    """M = 128: two 64-row conv blocks per strip (cv_gy = 2), four
    tickets per node, two staging passes in the dW role."""
    shape = (2, 128) + BASE[2:]
    _check(ext, Case(shape, torch.float64), _ring(2), dual, first=False)


@requires_gpu
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_dw_edge_tiles(ext, dtype):
    """H = 20 is no multiple of the dW role's 16 x 16 tile: threads past
    H must not step anything. M = 24 leaves the conv role's last wave
    without rows."""
    shape = (3, 24, 12, 5, 2, 20, 10)
    _check(ext, Case(shape, dtype), _ring(3), True)


@requires_gpu
def test_mnist_shape_one_node(ext):
    """The model's own layer shape (IMG 28, F 3, H 64): 27 conv blocks
    per node and 728 ticketed elements, three per thread."""
    shape = (2, 16, 28, 5, 3, 64, 10)
    _check(ext, Case(shape, torch.float64), _ring(2), True)


@requires_gpu
@pytest.mark.parametrize("dual", [True, False])
def test_fallback(ext, dual):
    """Seventeen nodes are one past the dispatch: the entry issues the
    old launches, steps theta_in in place, leaves theta_out alone and
    says so."""
    L = 17
    shape = (L,) + BASE[1:]
    assert not _fused_for(ext, shape, torch.float64)
    assert _fused_for(ext, (16,) + BASE[1:], torch.float64)
    # per-tile gradient slabs keep the step launch too
    assert not ext.bwd_step_fused_for(3, 16, 32, 16, 2, 5, 12, 8, 2)
    case = Case(shape, torch.float64)
    csr = _csr(_ring(L), torch.device("cuda"))
    old = _reference(ext, case, case.state, None, csr, dual, 0, 0.0,
                     False, 3)
    theta_out = torch.full_like(case.state["theta"], float("nan"))
    new, fused = _new(ext, case, case.state, theta_out, None, csr, dual,
                      0, 0.0, False, 3)
    torch.cuda.synchronize()
    assert not fused
    assert torch.isnan(theta_out).all()
    for k in ("theta", "duals", "s", "m", "v", "grad"):
        assert torch.equal(new[k], old[k]), k


@requires_gpu
def test_driver_rounds(tmp_path):
    """Three rounds of DiNNOStackedDriver on a ring of four, the fused
    path against NDTA_BWD_STEP=0, each in a fresh process (the switch is
    read once per process). eng.theta stays the same tensor object."""
    procs = {}
    for name, switch in (("old_a", "0"), ("old_b", "0"), ("new", None)):
        env = {**os.environ, "PYTHONPATH": os.pathsep.join(
            [ROOT, os.environ.get("PYTHONPATH", "")])}
        env.pop("NDTA_BWD_STEP", None)
        if switch is not None:
            env["NDTA_BWD_STEP"] = switch
        procs[name] = subprocess.Popen(
            [sys.executable, os.path.join(HERE, "bwd_step_checks.py"),
             str(tmp_path / f"{name}.pt")],
            env=env, cwd=ROOT, stdout=subprocess.PIPE,
            stderr=subprocess.STDOUT, text=True)
    out = {}
    for name, p in procs.items():
        log, _ = p.communicate(timeout=600)
        assert p.returncode == 0, log[-2000:]
        out[name] = torch.load(tmp_path / f"{name}.pt")
    assert out["new"]["fused"] and not out["old_a"]["fused"]
    for name in out:
        assert out[name]["same_theta_object"], name
        assert out[name]["grad_zero"], name
    for what in ("theta", "duals"):
        noise = (out["old_a"][what] - out["old_b"][what]).abs().max().item()
        diff = (out["new"][what] - out["old_a"][what]).abs().max().item()
        print(f"{what}: old-vs-old {noise:.3e}  new-vs-old {diff:.3e}")
        assert diff <= 10 * noise, what
