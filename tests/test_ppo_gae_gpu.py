"""GPU tests of GAE(lambda): ``ext.ppo_gae`` (ops/hip/advantage.hip)
against the torch mirror evaluated in fp64 on the same inputs, its
launch-to-launch determinism and argument checks, and one DiNNO round of
a ``DistPPOProblem`` with ``gae_lambda`` and ``critic_target: "lambda"``
under both rollout engines."""

import pytest
import torch

import ppo_gae_checks as gchk
import ppo_rollout_checks as chk
from nn_distributed_training_amd.rl import advantages as gae
from nn_distributed_training_amd.rl.ppo_optimizers import DiNNOPPO

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(
    not torch.cuda.is_available(), reason="needs MI355X"
)


@pytest.fixture
def dtype(request):
    prev = torch.get_default_dtype()
    torch.set_default_dtype(request.param)
    yield request.param
    torch.set_default_dtype(prev)


both_dtypes = pytest.mark.parametrize(
    "dtype", [torch.float64, torch.float32], indirect=True,
    ids=["fp64", "fp32"],
)


def _dev():
    return torch.device("cuda")


# (L, M, ep_len)
SHAPES = [
    (3, 70, 30),        # truncated last episode
    (1, 2, 1),          # every episode one step, the smallest legal M
    (2, 65, 65),        # one episode, one element past a wave
    (3, 300, 257),      # an episode past a 256-thread stride + a cut 43
    (8, 600, 100),      # the default workload's batch at the node limit
    (1, 16384, 4096),   # the largest batch whose advantages wait in LDS
    (2, 16385, 4096),   # the smallest that waits in global memory
]
LAMS = [0.0, 0.95, 1.0]

_REF = {}


def _reference(L, M, ep_len, dtype, per_node, lam):
    """Inputs (CPU) and the mirror's (adv, ret) in fp64, computed once
    per case and shared by the tests; never modified."""
    key = (L, M, ep_len, dtype, per_node, lam)
    if key not in _REF:
        v, rews = gchk.kernel_inputs(L, M, dtype, per_node)
        A, ret = gae.gae_advantages_torch(
            v, rews, gchk.uniform_lens(M, ep_len), gchk.GAMMA, lam)
        _REF[key] = (v, rews, gae.normalize_advantages(A), ret)
    return _REF[key]


def _launch(ext, v, rews, M, ep_len, lam, with_ret=True):
    L = v.shape[0]
    adv = torch.full((L * M,), float("nan"), device=v.device,
                     dtype=v.dtype)
    ret = torch.full_like(adv, float("nan")) if with_ret else None
    ext.ppo_gae(v.reshape(-1), rews.reshape(-1),
                M if rews.dim() == 2 else 0, adv, ret, M, ep_len,
                gchk.GAMMA, lam)
    return adv.view(L, M), None if ret is None else ret.view(L, M)


@requires_gpu
@both_dtypes
@pytest.mark.parametrize("lam", LAMS)
@pytest.mark.parametrize("per_node", [False, True],
                         ids=["rews_M", "rews_LM"])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_kernel_matches_the_mirror(dtype, shape, per_node, lam):
    from nn_distributed_training_amd.ops import get_ext

    L, M, ep_len = shape
    v, rews, want_adv, want_ret = _reference(
        L, M, ep_len, dtype, per_node, lam)
    adv, ret = _launch(get_ext(), v.to(_dev()), rews.to(_dev()), M,
                       ep_len, lam)
    adv, ret = adv.cpu(), ret.cpu()
    assert adv.dtype == dtype and ret.dtype == dtype
    print(f"max |adv - mirror| = "
          f"{(adv.double() - want_adv).abs().max():.3e}, max |ret - "
          f"mirror| = {(ret.double() - want_ret).abs().max():.3e}")
    torch.testing.assert_close(adv, want_adv.to(dtype), **chk.TOL[dtype])
    torch.testing.assert_close(ret, want_ret.to(dtype), **chk.TOL[dtype])
    if ep_len == 1:
        r = rews.expand(L, M) - v.double()
        torch.testing.assert_close(
            adv, gchk.normalize(r).to(dtype), **chk.TOL[dtype])


@requires_gpu
@both_dtypes
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_launches_are_bit_identical_and_ret_is_optional(dtype, shape):
    from nn_distributed_training_amd.ops import get_ext

    L, M, ep_len = shape
    v, rews, _, _ = _reference(L, M, ep_len, dtype, True, 0.95)
    v, rews = v.to(_dev()), rews.to(_dev())
    adv1, ret1 = _launch(get_ext(), v, rews, M, ep_len, 0.95)
    adv2, ret2 = _launch(get_ext(), v, rews, M, ep_len, 0.95)
    adv3, ret3 = _launch(get_ext(), v, rews, M, ep_len, 0.95,
                         with_ret=False)
    assert torch.isfinite(adv1).all() and torch.isfinite(ret1).all()
    assert torch.equal(adv1, adv2) and torch.equal(ret1, ret2)
    assert ret3 is None and torch.equal(adv1, adv3)


@requires_gpu
def test_out_of_range_arguments_raise_and_launch_nothing():
    from nn_distributed_training_amd.ops import get_ext

    ext = get_ext()
    dev = _dev()
    v = torch.randn(2, 8, device=dev, dtype=torch.float64)
    rews = torch.randn(8, device=dev, dtype=torch.float64)
    adv = torch.full((16,), 7.0, device=dev, dtype=torch.float64)
    ret = torch.full((16,), 7.0, device=dev, dtype=torch.float64)
    bad = [
        # M = 1: no unbiased std
        (v.reshape(-1)[:2], rews[:1], 0, adv[:2], ret[:2], 1, 1),
        # ep_len = 0, and one past the limit
        (v.reshape(-1), rews, 0, adv, ret, 8, 0),
        (v.reshape(-1), rews, 0, adv, ret, 8, gae.MAX_EP_LEN + 1),
        # dtype mismatches: adv, ret, rews
        (v.reshape(-1), rews, 0, adv.float(), ret, 8, 4),
        (v.reshape(-1), rews, 0, adv, ret.float(), 8, 4),
        (v.reshape(-1), rews.float(), 0, adv, ret, 8, 4),
        # CPU tensors
        (v.reshape(-1).cpu(), rews.cpu(), 0, adv.cpu(), ret.cpu(), 8, 4),
        (v.reshape(-1), rews.cpu(), 0, adv, ret, 8, 4),
        # a stride that does not fit the reward tensor
        (v.reshape(-1), rews, 8, adv, ret, 8, 4),
        # non-contiguous values
        (torch.randn(16, 2, device=dev, dtype=torch.float64)[:, 0], rews,
         0, adv, ret, 8, 4),
    ]
    for args in bad:
        with pytest.raises(RuntimeError):
            ext.ppo_gae(*args, gchk.GAMMA, 0.95)
    with pytest.raises(RuntimeError):
        ext.ppo_gae(v.reshape(-1), rews, 0, adv, ret, 8, 4, gchk.GAMMA,
                    1.5)
    torch.cuda.synchronize()
    assert (adv == 7.0).all() and (ret == 7.0).all()

    # the Python layer turns the same mistakes into ValueError
    for kwargs in [
        dict(v=v[:, :1], rews=rews[:1], ep_len=1),
        dict(v=v, rews=rews, ep_len=0),
        dict(v=v, rews=rews.float(), ep_len=4),
        dict(v=v.cpu(), rews=rews.cpu(), ep_len=4),
        dict(v=v.half(), rews=rews, ep_len=4),
        dict(v=v, rews=rews[:5], ep_len=4),
    ]:
        with pytest.raises(ValueError):
            gae.gae_advantages_hip(gamma=gchk.GAMMA, lam=0.95, **kwargs)
    with pytest.raises(ValueError):
        gae.gae_advantages_hip(v, rews, 4, gchk.GAMMA, -0.1)


# ----------------------------------------------------------------------
ROUND_CONF = {
    "verbose": False, "rho_init": 0.2, "primal_iterations": 3,
    "expected_iterations": 10, "primal_lr_start": 1e-3,
    "primal_lr_finish": 1e-4, "grad_engine": "stacked",
}


def _autograd_grads(pr):
    rows = []
    for i in range(pr.N):
        for p in pr.node_parameters(i):
            p.grad = None
        pr.local_batch_loss(i).backward()
        rows.append(
            torch.cat([p.grad.reshape(-1) for p in pr.node_parameters(i)])
        )
    return torch.stack(rows)


def _check_buffers(pr, rews, dtype):
    """``buf[i]["adv"]``/``["vtarg"]`` against the mirror on ``rews`` and
    the critic modules' values."""
    with torch.no_grad():
        v = torch.stack([
            pr.critics[i](pr.buf[i]["obs"]).squeeze(-1)
            for i in range(pr.N)
        ])
    A, ret = gae.gae_advantages_torch(
        v, rews, [30, 30, 10], pr.conf["gamma"], 0.95)
    adv = gae.normalize_advantages(A).to(dtype)
    for i in range(pr.N):
        b = pr.buf[i]
        assert b["adv"].shape == (70,) and b["adv"].dtype == dtype
        print(f"node {i}: max |adv - mirror| = "
              f"{(b['adv'] - adv[i]).abs().max():.3e}, max |vtarg - "
              f"mirror| = {(b['vtarg'] - ret[i].to(dtype)).abs().max():.3e}")
        torch.testing.assert_close(b["adv"], adv[i], **chk.TOL[dtype])
        torch.testing.assert_close(b["vtarg"], ret[i].to(dtype),
                                   **chk.TOL[dtype])


@pytest.fixture
def kernel_calls(monkeypatch):
    """Counts the launches ``DistPPOProblem`` asks of the kernel."""
    calls = []
    real = gae.gae_advantages_hip

    def spy(*args, **kwargs):
        calls.append(1)
        return real(*args, **kwargs)

    monkeypatch.setattr(gae, "gae_advantages_hip", spy)
    return calls


@requires_gpu
@both_dtypes
def test_round_with_gae_on_the_device_rollout(dtype, kernel_calls):
    pr = gchk.make_problem((16, 16), _dev(), rollout_engine="device",
                           gae_lambda=0.95, critic_target="lambda")
    opt = DiNNOPPO(pr, dict(ROUND_CONF))
    eng = opt.engine
    assert eng is not None and pr.value_engine is eng
    pr.rollout()
    assert len(kernel_calls) == 1
    ro = pr.device_buf
    assert ro["rews"].shape == (70,)
    _check_buffers(pr, ro["rews"], dtype)
    assert pr.buf[0]["vtarg"].data_ptr() == ro["vtarg"].data_ptr()

    # the engine regresses the critic on vtarg: its gradients are the
    # per-node autograd of local_batch_loss on the same buffers
    eng.load_device_rollout(ro)
    assert eng.vtarg.data_ptr() == ro["vtarg"].data_ptr()
    assert eng.rtgs.data_ptr() == ro["rtgs"].data_ptr()
    got = eng.grads(chk.theta_stack(pr)).clone()
    ref = _autograd_grads(pr)
    print(f"max |grad - autograd| = {(got - ref).abs().max():.3e}, "
          f"max |autograd| = {ref.abs().max():.3e}")
    for i in range(pr.N):
        torch.testing.assert_close(got[i], ref[i], **chk.TOL[dtype])

    before = chk.theta_stack(pr).clone()
    opt.step_round(0)
    after = chk.theta_stack(pr)
    assert torch.isfinite(after).all()
    assert not torch.equal(after, before)


@requires_gpu
@both_dtypes
def test_host_rollout_with_the_stacked_engine_reaches_the_kernel(
        dtype, kernel_calls):
    pr = gchk.make_problem((16, 16), _dev(), gae_lambda=0.95,
                           critic_target="lambda")
    opt = DiNNOPPO(pr, dict(ROUND_CONF))
    pr.rollout()
    assert pr.device_buf is None and len(kernel_calls) == 1
    rews = torch.stack([pr.buf[i]["rews"] for i in range(pr.N)])
    assert rews.shape == (pr.N, 70) and rews.dtype == torch.float64
    _check_buffers(pr, rews, dtype)
    opt.step_round(0)
    assert torch.equal(opt.engine.vtarg.view(pr.N, 70)[1],
                       pr.buf[1]["vtarg"])
    assert torch.isfinite(chk.theta_stack(pr)).all()


@requires_gpu
def test_gpu_problem_without_an_engine_uses_the_mirror(kernel_calls):
    prev = torch.get_default_dtype()
    torch.set_default_dtype(torch.float32)
    try:
        pr = gchk.make_problem((16, 16), _dev(), gae_lambda=0.95,
                               critic_target="lambda")
        pr.rollout()
        assert len(kernel_calls) == 0
        rews = torch.stack([pr.buf[i]["rews"] for i in range(pr.N)])
        _check_buffers(pr, rews, torch.float32)
    finally:
        torch.set_default_dtype(prev)
