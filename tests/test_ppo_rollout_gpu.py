"""GPU tests of the on-device rollout: ``ext.ppo_rollout`` through
``DeviceRollout`` against ``SimpleTagEnv``, the actor modules and
``rollout_host_mirror``, and one optimizer round with
``rollout_engine="device"``. The kernel runs once per (hidden, dtype)
case; the tests share its output."""

import numpy as np
import pytest
import torch
from torch.distributions import MultivariateNormal

import ppo_rollout_checks as chk
from nn_distributed_training_amd.rl.device_rollout import (
    DeviceRollout,
    gaussian_logp,
    rollout_host_mirror,
    set_env_state,
)
from nn_distributed_training_amd.rl.ppo_optimizers import (
    build_ppo_optimizer,
)

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


_CASES = {}


def _case(hidden, dtype):
    """(problem, resets, eps, kernel output) of one case, run once."""
    key = (hidden, dtype)
    if key not in _CASES:
        pr = chk.make_problem(hidden, _dev(), rollout_engine="device")
        resets, eps = chk.case_inputs(pr, dtype)
        out = pr.device_rollout.run(chk.theta_stack(pr), resets, eps)
        torch.cuda.synchronize()
        _CASES[key] = (pr, resets, eps, out)
    return _CASES[key]


@requires_gpu
@both_dtypes
@all_hiddens
def test_teacher_forced_step_parity(dtype, hidden):
    pr, _, _, out = _case(hidden, dtype)
    assert out["obs"].dtype == dtype and out["rews"].dtype == torch.float64
    stats = chk.assert_teacher_forced(pr, out, dtype)
    assert stats["steps"] == 70


@requires_gpu
@both_dtypes
@all_hiddens
def test_policy_parity(dtype, hidden):
    pr, _, eps, out = _case(hidden, dtype)
    Mb, ep_len = out["M"], out["ep_len"]
    # eps [E, ep_len, N, A] -> the [N*M, A] row layout
    eps_rows = torch.cat([
        eps[:, :, l].reshape(-1, 5)[:Mb] for l in range(chk.N)
    ]).to(_dev())
    for l in range(chk.N):
        s = slice(l * Mb, (l + 1) * Mb)
        with torch.no_grad():
            mean = pr.actors[l](out["obs"][s])
        got = out["acts"][s] - chk.SD * eps_rows[s]
        print(f"node {l}: max |mean - ref| = "
              f"{(got - mean).abs().max():.3e}")
        torch.testing.assert_close(got, mean, **chk.TOL[dtype])
        logp = MultivariateNormal(mean, pr.cov_mat).log_prob(
            out["acts"][s])
        torch.testing.assert_close(out["logp"][s], logp,
                                   **chk.TOL[dtype])


@requires_gpu
@both_dtypes
@all_hiddens
def test_returns_and_layout(dtype, hidden):
    pr, resets, eps, out = _case(hidden, dtype)
    Mb, ep_len = out["M"], out["ep_len"]
    E = 3
    assert (Mb, ep_len) == (70, 30)
    rews = out["rews"].cpu()
    # rtgs: the host recursion on the device rewards, per episode; the
    # truncated last episode (10 steps) neither leaks nor receives
    want = torch.tensor(
        chk.episode_rtgs(rews, pr.conf["gamma"], Mb, ep_len)).to(dtype)
    for l in range(chk.N):
        torch.testing.assert_close(
            out["rtgs"][l * Mb:(l + 1) * Mb].cpu(), want,
            **chk.TOL[dtype])
    last = torch.tensor(
        chk.episode_rtgs(rews[60:], pr.conf["gamma"], 10, 10)).to(dtype)
    torch.testing.assert_close(out["rtgs"][60:70].cpu(), last,
                               **chk.TOL[dtype])
    sums = torch.stack([rews[e * ep_len:(e + 1) * ep_len].sum()
                        for e in range(E)])
    torch.testing.assert_close(out["ep_rew"].cpu(), sums,
                               **chk.TOL[torch.float64])
    # row of (node l, episode e, step t) is l*M + e*ep_len + t: the
    # log-prob there is the one of eps[e, t, l], and every episode's
    # first observation is the one of its reset positions
    env = pr.env
    for e in range(E):
        set_env_state(env, resets[e, :chk.N], resets[e, chk.N])
        first = torch.as_tensor(env._observations()).to(dtype)
        r0 = chk.rows(e, 0, Mb, ep_len)
        torch.testing.assert_close(out["obs"][r0].cpu(), first,
                                   rtol=0, atol=0)
        for t in range(min(ep_len, Mb - e * ep_len)):
            r = chk.rows(e, t, Mb, ep_len)
            torch.testing.assert_close(
                out["logp"][r].cpu(),
                gaussian_logp(eps[e, t], chk.COV), **chk.TOL[dtype])


@requires_gpu
@all_hiddens
def test_whole_rollout_matches_host_mirror_fp64(hidden):
    """One 30-step episode from spread resets (no contacts) against the
    mirror with the same resets and noise. 30 steps compound, so the
    bound is 1e-8, not the per-op table."""
    pr = chk.make_problem(hidden, _dev(), rollout_engine="device",
                          M=30, ep=30)
    resets = np.array([[[0.7, 0.7], [-0.6, 0.6], [0.6, -0.5],
                        [0.0, 0.1]]])
    eps = chk.noise(1, 30, torch.float64, seed=14)
    ref = rollout_host_mirror(pr, resets, eps)
    gap = chk.min_gap(pr.env, ref)
    print(f"smallest gap between two bodies: {gap:.3f}")
    assert gap > 0.1  # the soft margin's force there: 1e-1 * e^-100
    out = pr.device_rollout.run(chk.theta_stack(pr), resets, eps)
    for key in ("obs", "acts", "logp", "rews", "rtgs", "ep_rew"):
        dev = (out[key] - ref[key]).abs().max().item()
        print(f"{key}: max |device - mirror| = {dev:.3e}")
    for key in ("obs", "acts", "logp", "rews", "rtgs", "ep_rew"):
        torch.testing.assert_close(out[key], ref[key], rtol=1e-8,
                                   atol=1e-8)


@requires_gpu
def test_device_rollout_rejects_unsupported_problems():
    prev = torch.get_default_dtype()
    torch.set_default_dtype(torch.float32)
    try:
        with pytest.raises(ValueError, match="layer widths"):
            chk.make_problem((16, 256), _dev(), rollout_engine="device")
        pr = chk.make_problem((16, 16), _dev())
        pr.env.n_obst = 9
        with pytest.raises(ValueError, match="obstacles"):
            DeviceRollout(pr)
    finally:
        torch.set_default_dtype(prev)


# ----------------------------------------------------------------------
ROUND_CONF = {
    "verbose": False, "rho_init": 0.2, "primal_iterations": 3,
    "expected_iterations": 10, "primal_lr_start": 1e-3,
    "primal_lr_finish": 1e-4,
}


@requires_gpu
@pytest.mark.parametrize("grad_engine", ["stacked", "torch"])
def test_round_with_device_rollout(grad_engine):
    prev = torch.get_default_dtype()
    torch.set_default_dtype(torch.float32)  # RL runs in fp32
    try:
        pr = chk.make_problem((16, 16), _dev(), rollout_engine="device")
        opt = build_ppo_optimizer(
            "dinno", pr, {**ROUND_CONF, "grad_engine": grad_engine})
        before = chk.theta_stack(pr).clone()
        pr.rollout()
        assert pr.total_timesteps == 70
        assert len(pr.ep_rew_history) == 1
        ro = pr.device_buf
        for i in range(pr.N):
            b = pr.buf[i]
            assert b["obs"].shape == (70, pr.env.obs_dim)
            assert b["obs"].data_ptr() == ro["obs"][i * 70].data_ptr()
            adv = b["rtgs"] - pr.critics[i](b["obs"]).squeeze(-1)
            adv = (adv - adv.mean()) / (adv.std() + 1e-10)
            torch.testing.assert_close(b["adv"], adv.detach(),
                                       **chk.TOL[torch.float32])
        opt.step_round(0)
        if grad_engine == "stacked":
            eng = opt.engine
            assert eng.obs.data_ptr() == ro["obs"].data_ptr()
            assert eng.acts.data_ptr() == ro["acts"].data_ptr()
            assert eng.old_logp.data_ptr() == ro["logp"].data_ptr()
            assert eng.rtgs.data_ptr() == ro["rtgs"].data_ptr()
        after = chk.theta_stack(pr)
        assert torch.isfinite(after).all()
        assert not torch.equal(after, before)
        pr.rollout()
        assert pr.total_timesteps == 140
        ev = pr.evaluate(episodes=2)
        assert isinstance(ev, float) and np.isfinite(ev)
    finally:
        torch.set_default_dtype(prev)
