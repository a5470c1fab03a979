"""CPU tests of partial-episode bootstrapping (``bootstrap_truncated``):
the torch mirror with ``v_last`` against an independent closed form, its
``lam = 1`` telescoping onto the bootstrapped rewards-to-go, the default
case, the fixed point of a constant reward stream, and a
``DistPPOProblem`` with the host rollout and per-node autograd."""

import pytest
import torch

import ppo_bootstrap_checks as bchk
import ppo_gae_checks as gchk
import ppo_rollout_checks as chk
from nn_distributed_training_amd.rl import advantages as gae
from nn_distributed_training_amd.rl import train_multi

GAMMA = gchk.GAMMA
LAMS = [0.0, 0.95, 1.0]
# ragged, with an episode of one step
EP_LENS = [7, 1, 12, 5]
L, M = 3, sum(EP_LENS)
TIGHT = dict(rtol=1e-12, atol=1e-12)


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


def _inputs(per_node):
    v, rews = gchk.kernel_inputs(L, M, torch.float64, per_node)
    return v, rews, bchk.kernel_v_last(L, len(EP_LENS), torch.float64)


@pytest.mark.parametrize("lam", LAMS)
@pytest.mark.parametrize("per_node", [False, True],
                         ids=["rews_M", "rews_LM"])
def test_mirror_matches_the_closed_form(per_node, lam):
    v, rews, v_last = _inputs(per_node)
    A, ret = gae.gae_advantages_torch(v, rews, EP_LENS, GAMMA, lam, v_last)
    want_A, want_ret, _ = bchk.closed_form(
        v, rews.expand(L, M), EP_LENS, GAMMA, lam, v_last)
    assert A.dtype == torch.float64 and A.shape == (L, M)
    print(f"max |A - closed form| = {(A - want_A).abs().max():.3e}")
    torch.testing.assert_close(A, want_A, **TIGHT)
    torch.testing.assert_close(ret, want_ret, **TIGHT)
    # the bootstrap moved something: the last step of every episode
    A0, _ = gae.gae_advantages_torch(v, rews, EP_LENS, GAMMA, lam)
    ends = torch.tensor(EP_LENS).cumsum(0) - 1
    torch.testing.assert_close(
        (A - A0)[:, ends], GAMMA * v_last, **TIGHT)


@pytest.mark.parametrize("per_node", [False, True],
                         ids=["rews_M", "rews_LM"])
def test_lambda_one_telescopes_onto_the_bootstrapped_rtgs(per_node):
    v, rews, v_last = _inputs(per_node)
    A, ret = gae.gae_advantages_torch(v, rews, EP_LENS, GAMMA, 1.0, v_last)
    _, _, want_rtg = bchk.closed_form(
        v, rews.expand(L, M), EP_LENS, GAMMA, 1.0, v_last)
    plain = torch.tensor([
        bchk._ragged_rtgs(rews.expand(L, M)[l], GAMMA, EP_LENS)
        for l in range(L)
    ], dtype=torch.float64)
    rtg_b = gae.bootstrap_rtgs(plain, v_last, EP_LENS, GAMMA)
    assert rtg_b.dtype == torch.float64 and rtg_b.shape == (L, M)
    torch.testing.assert_close(rtg_b, want_rtg, **TIGHT)
    torch.testing.assert_close(ret, rtg_b, **TIGHT)
    torch.testing.assert_close(A, rtg_b - v, **TIGHT)
    # the cached discounts serve a second call, and leave it unchanged
    assert torch.equal(
        gae.bootstrap_rtgs(plain, v_last, EP_LENS, GAMMA), rtg_b)
    # fp32 rewards-to-go come back as fp32
    assert gae.bootstrap_rtgs(
        plain.float(), v_last.float(), EP_LENS, GAMMA
    ).dtype == torch.float32
    with pytest.raises(ValueError):
        gae.bootstrap_rtgs(plain, v_last[:, :-1], EP_LENS, GAMMA)
    with pytest.raises(ValueError):
        gae.bootstrap_rtgs(plain, v_last, EP_LENS[:-1] + [4], GAMMA)


@pytest.mark.parametrize("lam", LAMS)
def test_no_bootstrap_is_todays_result(lam):
    v, rews, v_last = _inputs(True)
    today = gae.gae_advantages_torch(v, rews, EP_LENS, GAMMA, lam)
    none = gae.gae_advantages_torch(v, rews, EP_LENS, GAMMA, lam,
                                    v_last=None)
    zeros = gae.gae_advantages_torch(v, rews, EP_LENS, GAMMA, lam,
                                     v_last=torch.zeros_like(v_last))
    for got in (none, zeros):
        assert torch.equal(got[0], today[0])
        assert torch.equal(got[1], today[1])
    # today's result is the closed form of tests/ppo_gae_checks.py
    want_A, _ = gchk.closed_form(v, rews, EP_LENS, GAMMA, lam)
    torch.testing.assert_close(today[0], want_A, **TIGHT)
    plain = torch.randn(L, M, dtype=torch.float64)
    assert torch.equal(
        gae.bootstrap_rtgs(plain, torch.zeros_like(v_last), EP_LENS, GAMMA),
        plain)
    with pytest.raises(ValueError):
        gae.gae_advantages_torch(v, rews, EP_LENS, GAMMA, lam,
                                 v_last=v_last[:, :2])


@pytest.mark.parametrize("lam", LAMS)
def test_fixed_point_of_a_constant_reward_stream(lam):
    """r = c for ever is worth c / (1 - gamma) at every step: a critic
    that says so has zero advantage everywhere once the ends bootstrap,
    and is off by the whole tail at every end while they do not."""
    c = -0.3
    vstar = c / (1 - GAMMA)
    v = torch.full((L, M), vstar, dtype=torch.float64)
    rews = torch.full((M,), c, dtype=torch.float64)
    v_last = torch.full((L, len(EP_LENS)), vstar, dtype=torch.float64)
    A, ret = gae.gae_advantages_torch(v, rews, EP_LENS, GAMMA, lam, v_last)
    # |vstar| = 30: 1e-12 relative to it
    fp = dict(rtol=0, atol=1e-12 * abs(vstar))
    torch.testing.assert_close(A, torch.zeros_like(A), **fp)
    torch.testing.assert_close(ret, v, **fp)
    A0, _ = gae.gae_advantages_torch(v, rews, EP_LENS, GAMMA, lam)
    ends = torch.tensor(EP_LENS).cumsum(0) - 1
    torch.testing.assert_close(
        A0[:, ends], torch.full((L, len(EP_LENS)), -GAMMA * vstar,
                                dtype=torch.float64), **fp)


# ----------------------------------------------------------------------
def _pair(**extra):
    """The same seeded problem with the key off and on, each after one
    rollout() from the same torch seed."""
    out = []
    for boot in (False, True):
        pr = gchk.make_problem((16, 16), torch.device("cpu"),
                               bootstrap_truncated=boot, **extra)
        torch.manual_seed(7)
        pr.rollout()
        out.append(pr)
    return out


def _cat(pr, key):
    return torch.cat([pr.buf[i][key] for i in range(pr.N)])


@both_dtypes
@pytest.mark.parametrize(
    "extra", [{}, {"gae_lambda": 0.95, "critic_target": "lambda"}],
    ids=["mc", "gae"])
def test_problem_with_the_host_rollout(dtype, extra):
    off, on = _pair(**extra)
    lam = extra.get("gae_lambda")
    ep_lens = gchk.uniform_lens(chk.M, chk.EP)
    assert ep_lens == [30, 30, 10]
    assert off.bootstrap_truncated is False
    assert on.bootstrap_truncated is True

    # bootstrapping consumes no randomness
    for key in ("obs", "acts", "logp", "rews"):
        assert torch.equal(_cat(off, key), _cat(on, key)), key
    assert off.ep_rew_history == on.ep_rew_history
    assert torch.equal(off.last_obs, on.last_obs)

    # off: today's buffers. The rewards-to-go are rollout()'s recursion
    # and, under the default estimator, adv its rtg - V normalisation
    assert set(off.buf[0]) == {"obs", "acts", "logp", "rtgs", "rews",
                               "adv"} | ({"vtarg"} if lam else set())
    assert set(on.buf[0]) == set(off.buf[0])
    for i in range(off.N):
        b = off.buf[i]
        want = torch.tensor(
            chk.episode_rtgs(b["rews"], GAMMA, chk.M, chk.EP)).to(dtype)
        assert torch.equal(b["rtgs"], want)
        if lam is None:
            with torch.no_grad():
                adv = want - off.critics[i](b["obs"]).squeeze(-1)
            adv = (adv - adv.mean()) / (adv.std() + 1e-10)
            assert torch.equal(b["adv"], adv)
    if lam is not None:
        with torch.no_grad():
            v = torch.stack([
                off.critics[i](off.buf[i]["obs"]).squeeze(-1)
                for i in range(off.N)
            ])
        rews = torch.stack([off.buf[i]["rews"] for i in range(off.N)])
        A, ret = gae.gae_advantages_torch(v, rews, ep_lens, GAMMA, lam)
        assert torch.equal(
            torch.stack([off.buf[i]["adv"] for i in range(off.N)]),
            gae.normalize_advantages(A).to(dtype))
        assert torch.equal(
            torch.stack([off.buf[i]["vtarg"] for i in range(off.N)]),
            ret.to(dtype))

    # on: the mirror's targets from the critic modules
    N, E = on.N, len(ep_lens)
    assert on.last_obs.shape == (N * E, on.env.obs_dim)
    assert on.last_obs.dtype == dtype
    assert on.last_obs.device == on.device
    rtg_b, adv, vtarg = bchk.module_targets(
        on, _cat(on, "obs"),
        torch.stack([on.buf[i]["rews"] for i in range(N)]),
        on.last_obs, ep_lens, lam)
    tol = chk.TOL[dtype]
    for i in range(N):
        b = on.buf[i]
        assert b["rtgs"].dtype == dtype and b["adv"].dtype == dtype
        print(f"node {i}: max |rtgs - ref| = "
              f"{(b['rtgs'] - rtg_b[i]).abs().max():.3e}, max |adv - "
              f"ref| = {(b['adv'] - adv[i]).abs().max():.3e}")
        torch.testing.assert_close(b["rtgs"], rtg_b[i].to(dtype), **tol)
        torch.testing.assert_close(b["adv"], adv[i].to(dtype), **tol)
        if lam is not None:
            torch.testing.assert_close(b["vtarg"], vtarg[i].to(dtype),
                                       **tol)
        # and they are not today's
        assert not torch.equal(b["rtgs"], off.buf[i]["rtgs"])
        assert not torch.equal(b["adv"], off.buf[i]["adv"])
    # the critic's loss runs on whatever the buffers hold
    assert torch.isfinite(on.local_batch_loss(0))


@both_dtypes
def test_last_obs_is_one_env_step_past_the_last_recorded_row(dtype):
    _, on = _pair()
    bchk.assert_last_obs_teacher_forced(
        on, _cat(on, "obs"), _cat(on, "acts"), on.last_obs, chk.M, chk.EP,
        dtype)


def test_validation_and_command_line():
    for bad in (1, 0, "yes", None, 1.0):
        with pytest.raises(ValueError, match="bootstrap_truncated"):
            gchk.make_problem((16, 16), torch.device("cpu"),
                              bootstrap_truncated=bad)
    parser = train_multi.build_parser()
    args = parser.parse_args([])
    assert args.bootstrap_truncated is False
    assert train_multi.conf_from_args(args)["bootstrap_truncated"] is False
    args = parser.parse_args(["--bootstrap-truncated", "--gae-lambda",
                              "0.95", "--critic-target", "lambda"])
    assert args.bootstrap_truncated is True
    conf = train_multi.conf_from_args(args)
    assert conf["bootstrap_truncated"] is True
    assert conf["gae_lambda"] == 0.95
