"""CPU tests of the device rollout's host side: ``rollout_host_mirror``
against ``SimpleTagEnv.step`` and the actor modules, the reset stream,
the ``rollout_engine`` switch, and - on the mirror's output - the
teacher-forced check that tests/test_ppo_rollout_gpu.py applies to the
kernel's, with the same seeds."""

import copy
import math

import pytest
import torch
from torch.distributions import MultivariateNormal

import ppo_rollout_checks as chk
from nn_distributed_training_amd.rl.device_rollout import (
    draw_resets,
    episode_shape,
    rollout_host_mirror,
    set_env_state,
)
from nn_distributed_training_amd.rl.envs import SimpleTagEnv


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


@both_dtypes
def test_mirror_reproduces_env_and_actors(dtype):
    pr = chk.make_problem((16, 16), torch.device("cpu"))
    resets, eps = chk.case_inputs(pr, dtype)
    out = rollout_host_mirror(pr, resets, eps)
    Mb, ep_len, E = episode_shape(pr.conf, pr.env)
    assert (Mb, ep_len, E) == (70, 30, 3)
    assert out["obs"].shape == (chk.N * Mb, pr.env.obs_dim)
    assert out["acts"].shape == (chk.N * Mb, 5)
    assert out["rews"].shape == (Mb,) and out["ep_rew"].shape == (E,)

    env = copy.deepcopy(pr.env)
    rews = []
    for e in range(E):
        set_env_state(env, resets[e, :chk.N], resets[e, chk.N])
        for t in range(min(ep_len, Mb - e * ep_len)):
            r = chk.rows(e, t, Mb, ep_len)
            obs_t = torch.as_tensor(env._observations(), dtype=dtype)
            assert torch.equal(out["obs"][r], obs_t)
            with torch.no_grad():
                mean = torch.stack(
                    [pr.actors[i](obs_t[i]) for i in range(chk.N)])
            acts = mean + chk.SD * eps[e, t]
            torch.testing.assert_close(out["acts"][r], acts,
                                       **chk.TOL[dtype])
            logp = MultivariateNormal(mean, pr.cov_mat).log_prob(acts)
            torch.testing.assert_close(out["logp"][r], logp,
                                       **chk.TOL[dtype])
            _, rew, _, _ = env.step(out["acts"][r].numpy())
            assert rew[0] == rew[1] == rew[2]
            rews.append(float(rew[0]))
    torch.testing.assert_close(
        out["rews"], torch.tensor(rews, dtype=torch.float64),
        rtol=0, atol=0)
    want = torch.tensor(
        chk.episode_rtgs(rews, pr.conf["gamma"], Mb, ep_len)).to(dtype)
    for l in range(chk.N):
        assert torch.equal(out["rtgs"][l * Mb:(l + 1) * Mb], want)
    for e in range(E):
        ep = rews[e * ep_len: min((e + 1) * ep_len, Mb)]
        assert float(out["ep_rew"][e]) == pytest.approx(
            math.fsum(ep), rel=1e-12)


@both_dtypes
@pytest.mark.parametrize("hidden", chk.HIDDENS, ids=str)
def test_gpu_cases_exercise_the_env_on_the_mirror(dtype, hidden):
    """The seeds of the GPU tests: with the mirror in the kernel's
    place, the teacher-forced check passes, skips at most 1% of the
    steps, and the batch holds a catch and a contact."""
    pr = chk.make_problem(hidden, torch.device("cpu"))
    resets, eps = chk.case_inputs(pr, dtype)
    out = rollout_host_mirror(pr, resets, eps)
    stats = chk.assert_teacher_forced(pr, out, dtype)
    assert stats["steps"] == 70


def test_draw_resets_consumes_the_env_stream_like_reset():
    env_a = SimpleTagEnv(num_predators=3, num_obstacles=2, seed=7)
    env_b = copy.deepcopy(env_a)
    E = 4
    got = draw_resets(env_a, E)
    for e in range(E):
        env_b.reset()
        assert (got[e, :3] == env_b.pred_pos).all()
        assert (got[e, 3] == env_b.prey_pos).all()
    assert (env_a.rng.bit_generator.state
            == env_b.rng.bit_generator.state)


def test_device_rollout_needs_a_gpu_problem():
    with pytest.raises(ValueError, match="needs a GPU problem"):
        chk.make_problem((16, 16), torch.device("cpu"),
                         rollout_engine="device")


def test_unknown_rollout_engine_is_an_error():
    with pytest.raises(ValueError, match="'host' or 'device'"):
        chk.make_problem((16, 16), torch.device("cpu"),
                         rollout_engine="gpu")


def test_host_is_the_default_rollout_engine():
    pr = chk.make_problem((16, 16), torch.device("cpu"))
    assert "rollout_engine" not in pr.conf
    assert pr.rollout_engine == "host" and pr.device_rollout is None
    assert pr.device_buf is None


def test_train_multi_help_lists_rollout_engine(capsys):
    from nn_distributed_training_amd.rl import train_multi

    with pytest.raises(SystemExit) as ex:
        train_multi.main(["--help"])
    assert ex.value.code == 0
    text = capsys.readouterr().out
    assert "--rollout-engine" in text
    assert "{host,device}" in text
