"""Shared pieces of tests/test_ppo_rollout.py (CPU, on the host mirror)
and tests/test_ppo_rollout_gpu.py (on the kernel): the test problem, its
seeded resets and noise, and the teacher-forced step check, which takes a
rollout in the ``[N*M, .]`` layout from either source."""

import copy
import math

import networkx as nx
import numpy as np
import torch

from nn_distributed_training_amd.rl.device_rollout import (
    episode_shape,
    set_env_state,
    state_from_obs,
)
from nn_distributed_training_amd.rl.dist_ppo import DistPPOProblem
from nn_distributed_training_amd.rl.envs import (
    SimpleTagEnv,
    mpe_collision_force,
)

# the table of tests/test_ppo_stacked_gpu.py
TOL = {torch.float64: dict(rtol=1e-10, atol=1e-10),
       torch.float32: dict(rtol=2e-4, atol=2e-5)}

N, N_OBST = 3, 2
M, EP = 70, 30  # episodes of 30, 30 and a truncated 10
HIDDENS = [(16, 16), (64, 64, 64)]
COV = 0.5
# a step whose host margin to one of the env's three discontinuous
# decisions is below this may be skipped; at most 1% of the steps
MARGIN = 1e-7
MAX_SKIP = 0.01


def make_problem(hidden, device, rollout_engine=None, M=M, ep=EP):
    """3 predators, 2 obstacles, distinct parameters per node. Built
    under the current default dtype."""
    torch.manual_seed(0)
    env = SimpleTagEnv(num_predators=N, num_obstacles=N_OBST, seed=0,
                       max_steps=100)
    conf = {"hidden": hidden, "verbose": False, "cov": COV,
            "timesteps_per_batch": M, "max_timesteps_per_episode": ep}
    if rollout_engine is not None:
        conf["rollout_engine"] = rollout_engine
    pr = DistPPOProblem(nx.wheel_graph(N), env, device, conf)
    for i in range(pr.N):
        with torch.no_grad():
            for p in pr.node_parameters(i):
                p.add_(0.1 * torch.randn_like(p))
    return pr


def crowded_resets(E, seed=19):
    """Start positions in [-0.3, 0.3]^2: entities start in contact range
    of each other."""
    rng = np.random.default_rng(seed)
    return rng.uniform(-0.3, 0.3, size=(E, N + 1, 2))


def noise(E, ep_len, dtype, seed=5):
    gen = torch.Generator().manual_seed(seed)
    return torch.randn(E, ep_len, N, 5, generator=gen,
                       dtype=torch.float64).to(dtype)


def theta_stack(pr):
    return torch.stack(
        [pr.node_vector(i).detach() for i in range(pr.N)]
    ).contiguous()


def rows(e, t, M, ep_len):
    """Rows of step ``t`` of episode ``e`` for nodes 0..N-1."""
    return [l * M + e * ep_len + t for l in range(N)]


def _host_margins(env):
    """Margins of the pre-step decisions of the prey heuristic in the
    env's current state: nearest-predator argmin, +-1.2 cut-offs."""
    d = np.sort(np.linalg.norm(env.pred_pos - env.prey_pos, axis=1))
    argmin = d[1] - d[0] if len(d) > 1 else np.inf
    bound = np.min(np.abs(np.abs(env.prey_pos) - 1.2))
    return min(argmin, bound)


def _overlaps(env):
    """True where a predator overlaps another predator or any entity
    overlaps an obstacle (dist < dist_min: a contact force of at least
    CONTACT_FORCE * CONTACT_MARGIN * log 2, not the soft margin's
    far-field tail, which is never exactly zero)."""
    pos = np.vstack([env.pred_pos, env.prey_pos[None]])
    sizes = [env.pred_size] * env.n + [env.prey_size]
    hit = False
    for a in range(env.n):
        for b in range(a + 1, env.n):
            delta = pos[a] - pos[b]
            dist = np.linalg.norm(delta)
            f = mpe_collision_force(delta, dist, sizes[a] + sizes[b])
            hit |= dist < sizes[a] + sizes[b] and np.abs(f).max() > 0
    for a in range(env.n + 1):
        for o in range(env.n_obst):
            delta = pos[a] - env.obst_pos[o]
            dist = np.linalg.norm(delta)
            f = mpe_collision_force(delta, dist,
                                    sizes[a] + env.obst_size)
            hit |= dist < sizes[a] + env.obst_size and np.abs(f).max() > 0
    return bool(hit)


def teacher_forced_check(pr, out, tol):
    """For every recorded step: set a host env to the state decoded from
    the rollout's observation row, apply the rollout's recorded actions,
    step, and compare with the rollout's next observation and this
    step's reward. No error accumulates, so ``tol`` is the per-op table.
    Returns counts; raises on a mismatch."""
    Mb, ep_len = out["M"], out["ep_len"]
    E = -(-Mb // ep_len)
    obs = out["obs"].detach().cpu()
    acts = out["acts"].detach().cpu().double().numpy()
    rews = out["rews"].detach().cpu()
    dtype = obs.dtype
    env = copy.deepcopy(pr.env)
    catch_d = env.pred_size + env.prey_size
    stats = dict(steps=0, skipped=0, catches=0, contacts=0,
                 max_obs_err=0.0, max_rew_err=0.0)
    for e in range(E):
        ln = min(ep_len, Mb - e * ep_len)
        for t in range(ln):
            r = rows(e, t, Mb, ep_len)
            set_env_state(env, *_reorder(state_from_obs(obs[r].numpy())))
            margin = _host_margins(env)
            stats["contacts"] += _overlaps(env)
            nobs, rew, _, info = env.step(acts[r])
            d = np.linalg.norm(env.pred_pos - env.prey_pos, axis=1)
            margin = min(margin, np.min(np.abs(d - catch_d)))
            stats["steps"] += 1
            if margin < MARGIN:
                stats["skipped"] += 1
                continue
            stats["catches"] += bool(info["caught"].any())
            got_r = rews[e * ep_len + t]
            want_r = torch.tensor(rew[0], dtype=torch.float64)
            stats["max_rew_err"] = max(
                stats["max_rew_err"], abs(float(got_r - want_r)))
            # the reward is a double on both sides; the state it is
            # computed from went through the observation's dtype
            torch.testing.assert_close(got_r, want_r, **tol)
            if t + 1 < ln:
                got = obs[rows(e, t + 1, Mb, ep_len)]
                want = torch.as_tensor(nobs).to(dtype)
                stats["max_obs_err"] = max(
                    stats["max_obs_err"],
                    float((got - want).abs().max()))
                torch.testing.assert_close(got, want, **tol)
    return stats


def min_gap(env, out):
    """Smallest distance between two bodies' surfaces (movable pairs and
    movable-obstacle) over every recorded step of a rollout."""
    Mb, ep_len = out["M"], out["ep_len"]
    obs = out["obs"].detach().cpu().numpy()
    sizes = [env.pred_size] * env.n + [env.prey_size]
    gap = np.inf
    for m in range(Mb):
        r = [l * Mb + m for l in range(N)]
        pred_pos, _, prey_pos, _ = state_from_obs(obs[r])
        pos = np.vstack([pred_pos, prey_pos[None]])
        for a in range(env.n + 1):
            for b in range(a + 1, env.n + 1):
                gap = min(gap, np.linalg.norm(pos[a] - pos[b])
                          - sizes[a] - sizes[b])
            for o in range(env.n_obst):
                gap = min(gap, np.linalg.norm(pos[a] - env.obst_pos[o])
                          - sizes[a] - env.obst_size)
    return float(gap)


def _reorder(state):
    """state_from_obs order -> set_env_state's argument order."""
    pred_pos, pred_vel, prey_pos, prey_vel = state
    return pred_pos, prey_pos, pred_vel, prey_vel


def assert_teacher_forced(pr, out, dtype):
    stats = teacher_forced_check(pr, out, TOL[dtype])
    print(f"teacher-forced: {stats}")
    assert stats["skipped"] <= MAX_SKIP * stats["steps"], stats
    # otherwise the crowded resets did not do their job
    assert stats["catches"] >= 1, stats
    assert stats["contacts"] >= 1, stats
    return stats


def episode_rtgs(rews, gamma, Mb, ep_len):
    """rollout()'s reverse recursion on a [M] reward vector, per
    episode."""
    rews = [float(r) for r in rews]
    out = []
    for e in range(-(-Mb // ep_len)):
        ep = rews[e * ep_len: min((e + 1) * ep_len, Mb)]
        run, acc = 0.0, []
        for r in reversed(ep):
            run = r + gamma * run
            acc.append(run)
        out.extend(reversed(acc))
    return out


def case_inputs(pr, dtype):
    """The GPU tests' explicit resets and noise for problem ``pr``."""
    Mb, ep_len, E = episode_shape(pr.conf, pr.env)
    return crowded_resets(E), noise(E, ep_len, dtype)


SD = math.sqrt(COV)
