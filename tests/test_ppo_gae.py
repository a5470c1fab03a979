"""CPU tests of GAE(lambda) in the PPO tree: the torch mirror
``gae_advantages_torch`` against the Monte-Carlo estimator (lambda = 1)
and an independent closed form, ``DistPPOProblem`` under ``gae_lambda``
and ``critic_target``, the config errors and the ``train_multi`` flags."""

import pytest
import torch
from torch.distributions import MultivariateNormal

import ppo_gae_checks as gchk
import ppo_rollout_checks as chk
from nn_distributed_training_amd.rl.advantages import (
    gae_advantages_torch,
    normalize_advantages,
    uniform_ep_len,
)
from nn_distributed_training_amd.rl.device_rollout import (
    rollout_host_mirror,
)

CPU = torch.device("cpu")
TOL64 = chk.TOL[torch.float64]


@pytest.fixture
def dtype(request):
    prev = torch.get_default_dtype()
    torch.set_default_dtype(request.param)
    yield request.param
    torch.set_default_dtype(prev)


fp64 = pytest.mark.parametrize(
    "dtype", [torch.float64], indirect=True, ids=["fp64"])
both_dtypes = pytest.mark.parametrize(
    "dtype", [torch.float64, torch.float32], indirect=True,
    ids=["fp64", "fp32"],
)


def _critic_values(pr, obs_rows, M):
    with torch.no_grad():
        return torch.stack([
            pr.critics[i](obs_rows[i * M:(i + 1) * M]).squeeze(-1)
            for i in range(pr.N)
        ])


# ----------------------------------------------------------------------
@fp64
@pytest.mark.parametrize("hidden", chk.HIDDENS, ids=str)
def test_lambda_one_is_the_monte_carlo_estimator(dtype, hidden):
    pr = chk.make_problem(hidden, CPU)
    resets, eps = chk.case_inputs(pr, dtype)
    out = rollout_host_mirror(pr, resets, eps)
    M, ep_len = out["M"], out["ep_len"]
    assert (M, ep_len) == (70, 30)
    v = _critic_values(pr, out["obs"], M)
    rtgs = out["rtgs"].view(pr.N, M)
    A, ret = gae_advantages_torch(
        v, out["rews"], gchk.uniform_lens(M, ep_len), pr.conf["gamma"],
        1.0)
    assert A.dtype == torch.float64 and A.shape == (pr.N, M)
    print(f"max |A - (rtg - V)| = {(A - (rtgs - v)).abs().max():.3e}, "
          f"max |ret - rtg| = {(ret - rtgs).abs().max():.3e}")
    torch.testing.assert_close(A, rtgs - v, **TOL64)
    torch.testing.assert_close(ret, rtgs, **TOL64)
    torch.testing.assert_close(
        normalize_advantages(A), gchk.normalize(rtgs - v), **TOL64)


RAGGED = [
    [30, 30, 10],          # the device rollout's layout
    [1, 7, 1, 12, 3],      # ragged, with episodes of one step
    [23],                  # the batch is one episode
    [1, 1],                # every episode one step: A = r - V
    [5, 9, 2, 9],
]


@pytest.mark.parametrize("lam", [0.0, 0.5, 0.95])
@pytest.mark.parametrize("ep_lens", RAGGED, ids=str)
@pytest.mark.parametrize("per_node", [True, False],
                         ids=["rews_LM", "rews_M"])
def test_mirror_equals_the_closed_form(lam, ep_lens, per_node):
    L, M = 3, sum(ep_lens)
    v, rews = gchk.kernel_inputs(L, M, torch.float64, per_node)
    A, ret = gae_advantages_torch(v, rews, ep_lens, gchk.GAMMA, lam)
    want_A, want_ret = gchk.closed_form(
        v, rews.expand(L, M), ep_lens, gchk.GAMMA, lam)
    torch.testing.assert_close(A, want_A, **TOL64)
    torch.testing.assert_close(ret, want_ret, **TOL64)
    if ep_lens == [1, 1]:
        torch.testing.assert_close(A, rews.expand(L, M) - v, **TOL64)
    if lam == 0.0:
        # the one-step TD residual: the value after the step, or
        # nothing at an episode's end
        s = 0
        for n in ep_lens:
            torch.testing.assert_close(
                A[:, s + n - 1],
                rews.expand(L, M)[:, s + n - 1] - v[:, s + n - 1],
                **TOL64)
            s += n


def test_mirror_takes_fp32_values_in_double():
    v, rews = gchk.kernel_inputs(2, 40, torch.float32, True)
    A, ret = gae_advantages_torch(v, rews, [25, 15], gchk.GAMMA, 0.95)
    A64, ret64 = gae_advantages_torch(
        v.double(), rews, [25, 15], gchk.GAMMA, 0.95)
    assert A.dtype == torch.float64
    assert torch.equal(A, A64) and torch.equal(ret, ret64)


def test_mirror_rejects_lengths_that_do_not_partition_the_batch():
    v, rews = gchk.kernel_inputs(1, 10, torch.float64, True)
    with pytest.raises(ValueError, match="do not partition"):
        gae_advantages_torch(v, rews, [4, 4], 0.99, 0.95)
    with pytest.raises(ValueError, match="do not partition"):
        gae_advantages_torch(v, rews, [10, 0], 0.99, 0.95)


def test_uniform_ep_len():
    assert uniform_ep_len([30, 30, 10]) == 30
    assert uniform_ep_len([30, 30, 30]) == 30
    assert uniform_ep_len([7]) == 7
    assert uniform_ep_len([30, 10, 30]) is None
    assert uniform_ep_len([10, 30]) is None


# ----------------------------------------------------------------------
def _mc_advantages(pr):
    """Today's estimator on the problem's buffers."""
    out = []
    for i in range(pr.N):
        b = pr.buf[i]
        with torch.no_grad():
            v = pr.critics[i](b["obs"]).squeeze(-1)
        adv = b["rtgs"] - v
        out.append((adv - adv.mean()) / (adv.std() + 1e-10))
    return out


def _recomputed(pr, ep_lens, lam):
    """(normalised advantages, lambda-returns) of the problem's buffers
    by the closed form, from ``buf[i]["rews"]`` and the critic modules."""
    M = sum(ep_lens)
    v = _critic_values(
        pr, torch.cat([pr.buf[i]["obs"] for i in range(pr.N)]), M)
    rews = torch.stack([pr.buf[i]["rews"] for i in range(pr.N)])
    A, ret = gchk.closed_form(v, rews, ep_lens, pr.conf["gamma"], lam)
    return gchk.normalize(A), ret


@both_dtypes
def test_problem_advantages_are_gae(dtype):
    pr = gchk.make_problem((16, 16), CPU, gae_lambda=0.95)
    pr.rollout()
    adv, _ = _recomputed(pr, [30, 30, 10], 0.95)
    mc = _mc_advantages(pr)
    gap = 0.0
    for i in range(pr.N):
        b = pr.buf[i]
        assert b["adv"].dtype == dtype and b["adv"].shape == (70,)
        assert b["rews"].dtype == torch.float64
        assert "vtarg" not in b
        torch.testing.assert_close(b["adv"], adv[i].to(dtype),
                                   **chk.TOL[dtype])
        gap = max(gap, float((b["adv"] - mc[i]).abs().max()))
    print(f"max |GAE(0.95) - Monte-Carlo| after normalisation: {gap:.3f}")
    assert gap > 0.1


@fp64
def test_problem_lambda_one_matches_the_default_path(dtype):
    pr = gchk.make_problem((16, 16), CPU, gae_lambda=1.0)
    pr.rollout()
    mc = _mc_advantages(pr)
    for i in range(pr.N):
        torch.testing.assert_close(pr.buf[i]["adv"], mc[i], **TOL64)


@fp64
def test_critic_target_lambda_regresses_on_the_lambda_returns(dtype):
    pr = gchk.make_problem((16, 16), CPU, gae_lambda=0.95,
                           critic_target="lambda")
    pr.rollout()
    _, ret = _recomputed(pr, [30, 30, 10], 0.95)
    clip, coef = pr.conf["clip"], pr.conf["critic_coef"]
    for i in range(pr.N):
        b = pr.buf[i]
        torch.testing.assert_close(b["vtarg"], ret[i], **TOL64)
        assert (b["vtarg"] - b["rtgs"]).abs().max() > 1e-3
        with torch.no_grad():
            logp = MultivariateNormal(
                pr.actors[i](b["obs"]), pr.cov_mat).log_prob(b["acts"])
            r = torch.exp(logp - b["logp"])
            actor = -torch.min(
                r * b["adv"],
                torch.clamp(r, 1 - clip, 1 + clip) * b["adv"]).mean()
            v = pr.critics[i](b["obs"]).squeeze(-1)
            critic = pr.local_batch_loss(i) - actor
        torch.testing.assert_close(
            critic, coef * ((v - ret[i]) ** 2).mean(), **TOL64)
        assert abs(float(critic - coef * ((v - b["rtgs"]) ** 2).mean())
                   ) > 1e-6


@both_dtypes
def test_default_config_is_todays_estimator_bit_for_bit(dtype):
    pr = gchk.make_problem((16, 16), CPU)
    assert pr.gae_lambda is None and pr.critic_target == "rtg"
    pr.rollout()
    mc = _mc_advantages(pr)
    for i in range(pr.N):
        b = pr.buf[i]
        assert torch.equal(b["adv"], mc[i])
        assert "vtarg" not in b
        # the per-step rewards are kept, and are the ones behind rtgs
        assert b["rews"].dtype == torch.float64 and b["rews"].shape == (70,)
        want = torch.tensor(chk.episode_rtgs(
            b["rews"], pr.conf["gamma"], 70, 30)).to(dtype)
        assert torch.equal(b["rtgs"], want)


def test_episode_lengths_are_the_ones_the_env_gave():
    """With env.max_steps below the episode limit the env ends the
    episodes: the lengths used are the real ones, 25, 25, 20."""
    prev = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        pr = gchk.make_problem((16, 16), CPU, gae_lambda=0.5)
        pr.env.max_steps = 25
        pr.rollout()
        adv, _ = _recomputed(pr, [25, 25, 20], 0.5)
        for i in range(pr.N):
            torch.testing.assert_close(pr.buf[i]["adv"], adv[i], **TOL64)
    finally:
        torch.set_default_dtype(prev)


# ----------------------------------------------------------------------
@pytest.mark.parametrize("lam", [-0.1, 1.5])
def test_gae_lambda_outside_the_unit_interval_is_an_error(lam):
    with pytest.raises(ValueError, match="gae_lambda"):
        gchk.make_problem((16, 16), CPU, gae_lambda=lam)


def test_unknown_critic_target_is_an_error():
    with pytest.raises(ValueError, match="'rtg' or 'lambda'"):
        gchk.make_problem((16, 16), CPU, gae_lambda=0.9,
                          critic_target="td")


def test_lambda_target_needs_a_gae_lambda():
    with pytest.raises(ValueError, match="needs a gae_lambda"):
        gchk.make_problem((16, 16), CPU, critic_target="lambda")


def test_train_multi_parser_takes_the_gae_flags():
    from nn_distributed_training_amd.rl import train_multi

    p = train_multi.build_parser()
    args = p.parse_args(["--gae-lambda", "0.95", "--critic-target",
                         "lambda"])
    conf = train_multi.conf_from_args(args)
    assert conf["gae_lambda"] == 0.95
    assert conf["critic_target"] == "lambda"
    conf = train_multi.conf_from_args(p.parse_args([]))
    assert conf["gae_lambda"] is None and conf["critic_target"] == "rtg"
    with pytest.raises(SystemExit):
        p.parse_args(["--critic-target", "td"])
