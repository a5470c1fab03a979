"""GPU tests of partial-episode bootstrapping: ``ext.ppo_gae`` with
``v_last`` against the torch mirror in fp64, ``ext.ppo_rollout``'s
``last_obs`` against the host env, ``StackedPPOEngine.values_last``
against the critic modules, and whole DiNNO rounds of a
``DistPPOProblem`` with ``bootstrap_truncated`` on the device rollout."""

import pytest
import torch

import ppo_bootstrap_checks as bchk
import ppo_gae_checks as gchk
import ppo_rollout_checks as chk
from nn_distributed_training_amd.rl import advantages as gae
from nn_distributed_training_amd.rl.device_rollout import (
    ACT_DIM,
    rollout_host_mirror,
)
from nn_distributed_training_amd.rl.ppo_optimizers import DiNNOPPO
from nn_distributed_training_amd.rl.stacked_ppo import StackedPPOEngine

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
all_hiddens = pytest.mark.parametrize("hidden", chk.HIDDENS, ids=str)


def _dev():
    return torch.device("cuda")


# (L, M, ep_len)
SHAPES = [
    (3, 70, 30),        # truncated last episode
    (1, 2, 1),          # every step is an episode's end
    (2, 65, 65),        # one episode, one element past a wave
    (3, 300, 257),      # an episode past a 256-thread stride + a cut 43
    (2, 16385, 4096),   # the advantages wait in global memory
]
LAMS = [0.0, 0.95, 1.0]

_REF = {}


def _reference(L, M, ep_len, dtype, per_node, lam):
    """Inputs (CPU) and the mirror's (adv, ret) in fp64, computed once
    per case and shared by the tests; never modified."""
    key = (L, M, ep_len, dtype, per_node, lam)
    if key not in _REF:
        v, rews = gchk.kernel_inputs(L, M, dtype, per_node)
        v_last = bchk.kernel_v_last(L, -(-M // ep_len), dtype)
        A, ret = gae.gae_advantages_torch(
            v, rews, gchk.uniform_lens(M, ep_len), gchk.GAMMA, lam, v_last)
        _REF[key] = (v, rews, v_last, gae.normalize_advantages(A), ret)
    return _REF[key]


def _launch(ext, v, rews, M, ep_len, lam, *v_last):
    """``ext.ppo_gae`` with its nine arguments of old, plus ``v_last``
    where one is given (positionally, or not at all)."""
    L = v.shape[0]
    adv = torch.full((L * M,), float("nan"), device=v.device,
                     dtype=v.dtype)
    ret = torch.full_like(adv, float("nan"))
    ext.ppo_gae(v.reshape(-1), rews.reshape(-1),
                M if rews.dim() == 2 else 0, adv, ret, M, ep_len,
                gchk.GAMMA, lam, *v_last)
    return adv.view(L, M), ret.view(L, M)


@requires_gpu
@both_dtypes
@pytest.mark.parametrize("lam", LAMS)
@pytest.mark.parametrize("per_node", [False, True],
                         ids=["rews_M", "rews_LM"])
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_gae_kernel_with_v_last_matches_the_mirror(dtype, shape, per_node,
                                                   lam):
    from nn_distributed_training_amd.ops import get_ext

    L, M, ep_len = shape
    v, rews, v_last, want_adv, want_ret = _reference(
        L, M, ep_len, dtype, per_node, lam)
    adv, ret = _launch(get_ext(), v.to(_dev()), rews.to(_dev()), M,
                       ep_len, lam, v_last.to(_dev()).reshape(-1))
    adv, ret = adv.cpu(), ret.cpu()
    assert adv.dtype == dtype and ret.dtype == dtype
    print(f"max |adv - mirror| = "
          f"{(adv.double() - want_adv).abs().max():.3e}, max |ret - "
          f"mirror| = {(ret.double() - want_ret).abs().max():.3e}")
    torch.testing.assert_close(adv, want_adv.to(dtype), **chk.TOL[dtype])
    torch.testing.assert_close(ret, want_ret.to(dtype), **chk.TOL[dtype])
    # the Python layer launches the same thing
    adv2, ret2 = gae.gae_advantages_hip(
        v.to(_dev()), rews.to(_dev()), ep_len, gchk.GAMMA, lam,
        v_last=v_last.to(_dev()))
    assert torch.equal(adv2.cpu(), adv) and torch.equal(ret2.cpu(), ret)


@requires_gpu
@both_dtypes
@pytest.mark.parametrize("shape", SHAPES, ids=str)
def test_gae_kernel_without_v_last_is_the_kernel_of_old(dtype, shape):
    from nn_distributed_training_amd.ops import get_ext

    ext = get_ext()
    L, M, ep_len = shape
    v, rews, v_last, _, _ = _reference(L, M, ep_len, dtype, True, 0.95)
    v, rews = v.to(_dev()), rews.to(_dev())
    nine = _launch(ext, v, rews, M, ep_len, 0.95)
    none = _launch(ext, v, rews, M, ep_len, 0.95, None)
    zeros = _launch(ext, v, rews, M, ep_len, 0.95,
                    torch.zeros(v_last.numel(), device=_dev(), dtype=dtype))
    assert torch.isfinite(nine[0]).all() and torch.isfinite(nine[1]).all()
    for got in (none, zeros):
        assert torch.equal(got[0], nine[0])
        assert torch.equal(got[1], nine[1])
    # and the nine-argument launch is the mirror without a bootstrap
    A, ret = gae.gae_advantages_torch(
        v.cpu(), rews.cpu(), gchk.uniform_lens(M, ep_len), gchk.GAMMA,
        0.95)
    torch.testing.assert_close(
        nine[0].cpu(), gae.normalize_advantages(A).to(dtype),
        **chk.TOL[dtype])
    torch.testing.assert_close(nine[1].cpu(), ret.to(dtype),
                               **chk.TOL[dtype])


@requires_gpu
@both_dtypes
@pytest.mark.parametrize("lam", LAMS)
@pytest.mark.parametrize("shape", [(3, 70, 30), (3, 300, 257)], ids=str)
def test_gae_kernel_fixed_point(dtype, shape, lam):
    """Constant rewards c, V = V_end = c / (1 - gamma): the lambda-return
    is V itself (the advantages are rounding noise, and normalising them
    says nothing)."""
    from nn_distributed_training_amd.ops import get_ext

    L, M, ep_len = shape
    c = -0.3
    vstar = c / (1 - gchk.GAMMA)
    E = -(-M // ep_len)
    v = torch.full((L, M), vstar, device=_dev(), dtype=dtype)
    rews = torch.full((M,), c, device=_dev(), dtype=torch.float64)
    v_last = torch.full((L * E,), vstar, device=_dev(), dtype=dtype)
    _, ret = _launch(get_ext(), v, rews, M, ep_len, lam, v_last)
    print(f"max |ret - v| = {(ret - v).abs().max():.3e}")
    torch.testing.assert_close(ret, v, **chk.TOL[dtype])
    # without the bootstrap every episode's end misses the tail
    _, ret0 = _launch(get_ext(), v, rews, M, ep_len, lam)
    ends = [min(s + ep_len, M) - 1 for s in range(0, M, ep_len)]
    torch.testing.assert_close(
        (ret0 - v)[:, ends],
        torch.full((L, E), -gchk.GAMMA * vstar, device=_dev(),
                   dtype=dtype), **chk.TOL[dtype])


@requires_gpu
def test_bad_v_last_raises_and_launches_nothing():
    from nn_distributed_training_amd.ops import get_ext

    ext = get_ext()
    dev = _dev()
    L, M, ep_len, E = 2, 8, 3, 3
    v = torch.randn(L, M, device=dev, dtype=torch.float64)
    rews = torch.randn(M, device=dev, dtype=torch.float64)
    adv = torch.full((L * M,), 7.0, device=dev, dtype=torch.float64)
    ret = torch.full((L * M,), 7.0, device=dev, dtype=torch.float64)
    good = torch.randn(L * E, device=dev, dtype=torch.float64)
    bad = [
        torch.randn(L * E + 1, device=dev, dtype=torch.float64),
        torch.randn(L * E - 1, device=dev, dtype=torch.float64),
        good.float(),
        good.cpu(),
        torch.randn(L * E, 2, device=dev, dtype=torch.float64)[:, 0],
    ]
    for v_last in bad:
        with pytest.raises(RuntimeError):
            ext.ppo_gae(v.reshape(-1), rews, 0, adv, ret, M, ep_len,
                        gchk.GAMMA, 0.95, v_last)
    torch.cuda.synchronize()
    assert (adv == 7.0).all() and (ret == 7.0).all()

    # the Python layer turns the same mistakes into ValueError
    for v_last in [good.view(L, E)[:, :2], good.view(E, L),
                   good.view(L, E).float(), good.view(L, E).cpu(), good]:
        with pytest.raises(ValueError):
            gae.gae_advantages_hip(v, rews, ep_len, gchk.GAMMA, 0.95,
                                   v_last=v_last)
    # a non-contiguous [L, E] view is fine there: it is made contiguous
    wide = torch.randn(L, 2 * E, device=dev, dtype=torch.float64)
    a1, _ = gae.gae_advantages_hip(v, rews, ep_len, gchk.GAMMA, 0.95,
                                   v_last=wide[:, ::2])
    a2, _ = gae.gae_advantages_hip(v, rews, ep_len, gchk.GAMMA, 0.95,
                                   v_last=wide[:, ::2].contiguous())
    assert torch.equal(a1, a2)


# ----------------------------------------------------------------------
_CASES = {}


def _case(hidden, dtype, M=chk.M, ep=chk.EP):
    """(problem, resets, eps, kernel output) of one case, run once."""
    key = (hidden, dtype, M, ep)
    if key not in _CASES:
        pr = chk.make_problem(hidden, _dev(), rollout_engine="device",
                              M=M, ep=ep)
        resets, eps = chk.case_inputs(pr, dtype)
        out = pr.device_rollout.run(chk.theta_stack(pr), resets, eps)
        torch.cuda.synchronize()
        _CASES[key] = (pr, resets, eps, out)
    return _CASES[key]


@requires_gpu
@both_dtypes
@all_hiddens
def test_last_obs_teacher_forced(dtype, hidden):
    pr, _, _, out = _case(hidden, dtype)
    assert (out["M"], out["ep_len"]) == (70, 30)
    assert out["last_obs"].shape == (chk.N * 3, pr.env.obs_dim)
    assert out["last_obs"].is_cuda and out["last_obs"].dtype == dtype
    bchk.assert_last_obs_teacher_forced(
        pr, out["obs"], out["acts"], out["last_obs"], 70, 30, dtype)


@requires_gpu
@both_dtypes
def test_last_obs_of_a_single_episode(dtype):
    pr, _, _, out = _case((16, 16), dtype, M=30, ep=30)
    assert (out["M"], out["ep_len"]) == (30, 30)
    assert out["last_obs"].shape == (chk.N, pr.env.obs_dim)
    bchk.assert_last_obs_teacher_forced(
        pr, out["obs"], out["acts"], out["last_obs"], 30, 30, dtype)


@requires_gpu
def test_last_obs_matches_the_host_mirror_fp64():
    prev = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        pr, resets, eps, out = _case((16, 16), torch.float64)
        ref = rollout_host_mirror(pr, resets, eps)
        assert ref["last_obs"].shape == out["last_obs"].shape
        err = (out["last_obs"] - ref["last_obs"]).abs().max().item()
        print(f"last_obs: max |device - mirror| = {err:.3e}")
        torch.testing.assert_close(out["last_obs"], ref["last_obs"],
                                   **chk.TOL[torch.float64])
    finally:
        torch.set_default_dtype(prev)


@requires_gpu
@both_dtypes
def test_rollout_without_last_obs_is_the_rollout_of_old(dtype):
    from nn_distributed_training_amd.ops import get_ext

    pr, resets, eps, out = _case((16, 16), dtype)
    dr = pr.device_rollout
    dev, N, M, ep_len, E = _dev(), chk.N, 70, 30, 3
    resets_t = torch.as_tensor(resets, dtype=torch.float64).to(dev)
    eps_t = eps.to(dev, dtype).contiguous()

    def launch(*last_obs):
        def mk(*shape, dt=dtype):
            return torch.full(shape, float("nan"), device=dev, dtype=dt)

        o = dict(obs=mk(N * M, dr.obs_dim), acts=mk(N * M, ACT_DIM),
                 logp=mk(N * M), rews=mk(M, dt=torch.float64),
                 rtgs=mk(N * M), ep_rew=mk(E, dt=torch.float64))
        get_ext().ppo_rollout(
            chk.theta_stack(pr), *dr._plan, resets_t, dr._obst, eps_t,
            o["obs"], o["acts"], o["logp"], o["rews"], o["rtgs"],
            o["ep_rew"], M, ep_len, chk.COV, float(pr.conf["gamma"]),
            dr._envp, *last_obs)
        return o

    last = torch.full((N * E, dr.obs_dim), float("nan"), device=dev,
                      dtype=dtype)
    old, none, with_last = launch(), launch(None), launch(last)
    for key in old:
        assert torch.isfinite(old[key]).all(), key
        assert torch.equal(old[key], none[key]), key
        assert torch.equal(old[key], with_last[key]), key
        assert torch.equal(old[key], out[key]), key
    assert torch.equal(last, out["last_obs"])

    # a last_obs the kernel cannot take launches nothing
    filled = torch.full_like(last, 7.0)
    bad = [filled[:-1], filled.to(torch.float32 if dtype == torch.float64
                                  else torch.float64),
           filled.cpu(), filled.t()]
    for lo in bad:
        with pytest.raises(RuntimeError):
            launch(lo)
    torch.cuda.synchronize()
    assert (filled == 7.0).all()


# ----------------------------------------------------------------------
@requires_gpu
@both_dtypes
@all_hiddens
@pytest.mark.parametrize("E", [1, 3])
def test_values_last_matches_the_critic_modules(dtype, hidden, E):
    pr = chk.make_problem(hidden, _dev())
    eng = StackedPPOEngine(pr)
    torch.manual_seed(3)
    pr.rollout()
    eng.load_rollout(pr.buf)
    theta = chk.theta_stack(pr)
    before = eng.values(theta)
    obs_ptr = eng.obs.data_ptr()
    gen = torch.Generator().manual_seed(17)
    last_obs = torch.randn(pr.N * E, pr.env.obs_dim, generator=gen,
                           dtype=torch.float64).to(_dev(), dtype)
    got = eng.values_last(theta, last_obs)
    assert got.shape == (pr.N, E) and got.dtype == dtype
    for i in range(pr.N):
        with torch.no_grad():
            ref = pr.critics[i](last_obs[i * E:(i + 1) * E]).squeeze(-1)
        print(f"node {i}: max |values_last - critic| = "
              f"{(got[i] - ref).abs().max():.3e}")
        torch.testing.assert_close(got[i], ref, **chk.TOL[dtype])
    # the loaded rollout and its M-row buffers are as they were
    assert eng.obs.data_ptr() == obs_ptr and eng.M == chk.M
    assert torch.equal(eng.values(theta), before)
    assert torch.equal(eng.values_last(theta, last_obs), got)


# ----------------------------------------------------------------------
ROUND_CONF = {
    "verbose": False, "rho_init": 0.2, "primal_iterations": 3,
    "expected_iterations": 10, "primal_lr_start": 1e-3,
    "primal_lr_finish": 1e-4,
}


@requires_gpu
@both_dtypes
@pytest.mark.parametrize("grad_engine", ["stacked", "torch"])
@pytest.mark.parametrize(
    "extra", [{}, {"gae_lambda": 0.95, "critic_target": "lambda"}],
    ids=["mc", "gae"])
def test_round_with_bootstrapping_on_the_device_rollout(dtype, grad_engine,
                                                        extra):
    lam = extra.get("gae_lambda")
    pr = gchk.make_problem((16, 16), _dev(), rollout_engine="device",
                           bootstrap_truncated=True, **extra)
    opt = DiNNOPPO(pr, {**ROUND_CONF, "grad_engine": grad_engine})
    assert (pr.value_engine is not None) == (grad_engine == "stacked")
    pr.rollout()
    ro = pr.device_buf
    N, M, E = pr.N, 70, 3
    assert pr.last_obs.data_ptr() == ro["last_obs"].data_ptr()
    assert pr.last_obs.shape == (N * E, pr.env.obs_dim)
    assert pr.last_obs.dtype == dtype and pr.last_obs.is_cuda
    bchk.assert_last_obs_teacher_forced(
        pr, ro["obs"], ro["acts"], pr.last_obs, M, 30, dtype)
    rtg_b, adv, vtarg = bchk.module_targets(
        pr, ro["obs"], ro["rews"], pr.last_obs, [30, 30, 10], lam)
    tol = chk.TOL[dtype]
    got = {k: ro[k].view(N, M).cpu() for k in ("rtgs", "adv")}
    want = {"rtgs": rtg_b, "adv": adv}
    if lam is not None:
        got["vtarg"] = ro["vtarg"].view(N, M).cpu()
        want["vtarg"] = vtarg
    else:
        assert "vtarg" not in ro
    for k in got:
        print(f"{k}: max |round - mirror| = "
              f"{(got[k].double() - want[k]).abs().max():.3e}")
    for k in got:
        assert got[k].dtype == dtype
        torch.testing.assert_close(got[k], want[k].to(dtype), **tol)
    # the per-node buffers are views of the same tensors
    assert pr.buf[1]["rtgs"].data_ptr() == ro["rtgs"][M].data_ptr()
    # and the tail is there: the plain rewards-to-go differ
    plain = torch.tensor(
        chk.episode_rtgs(ro["rews"].cpu(), pr.conf["gamma"], M, 30))
    assert (got["rtgs"][0].double() - plain).abs().max() > 1e-3

    before = chk.theta_stack(pr).clone()
    opt.step_round(0)
    if grad_engine == "stacked":
        assert opt.engine.rtgs.data_ptr() == ro["rtgs"].data_ptr()
    after = chk.theta_stack(pr)
    assert torch.isfinite(after).all()
    assert not torch.equal(after, before)
