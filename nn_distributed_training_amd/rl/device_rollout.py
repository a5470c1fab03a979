"""One batch of ``SimpleTagEnv`` episodes in a single kernel launch.

``DistPPOProblem.rollout()`` steps one numpy env on the host and calls
every node's actor module once per step. In this env an episode ends only
at its step limit, so the episodes of a batch of ``M =
timesteps_per_batch`` steps are known before it starts: episode ``e``
covers steps ``[e*ep_len, e*ep_len + len_e)`` with ``ep_len =
min(max_timesteps_per_episode, env.max_steps)`` and ``len_e = min(ep_len,
M - e*ep_len)`` (the last one may be truncated, as ``rollout()``
truncates it). ``ext.ppo_rollout`` (ops/hip/rollout.hip) runs one block
per episode - actor forward, Gaussian action, log-prob, prey heuristic,
physics, reward, rewards-to-go - and writes the ``[N*M, .]`` tensors that
``StackedPPOEngine`` consumes: node ``l``'s step ``t`` of episode ``e`` is
row ``l*M + e*ep_len + t``. ``rollout_engine: "device"`` of
``DistPPOProblem`` selects it. Every such end is a truncation, so the
kernel also writes ``last_obs [N*E, obs_dim]``: row ``l*E + e`` is node
``l``'s observation after episode ``e``'s last step, what ``env.step``
returned there, for ``bootstrap_truncated`` (rl/advantages.py).

The randomness comes in as tensors: reset positions drawn from
``env.rng`` in ``SimpleTagEnv.reset()``'s order (the env's stream is
consumed as the host rollout consumes it), and standard-normal noise
``eps [E, ep_len, N, A]`` from one ``torch.randn``; the action is ``mean
+ sqrt(cov)*eps``. That is the distribution ``MultivariateNormal(mean,
cov*I).sample()`` draws from, but not its random stream: a device run and
a host run with the same seed see different actions.

:func:`rollout_host_mirror` is the same rollout in plain numpy/torch on a
real ``SimpleTagEnv``: the documentation of what the kernel computes and
the oracle of the tests.
"""

from __future__ import annotations

import copy
import math

import numpy as np
import torch

from . import envs
from .stacked_ppo import shifted_plan
from ..ops.stacked import ACT_IDS

# the kernel's compile-time limits (ops/hip/rollout.hip)
MAX_NODES = 8
MAX_OBSTACLES = 8
MAX_WIDTH = 128
MAX_LAYERS = 8
MAX_EP_LEN = 4096
ACT_DIM = 5


def episode_shape(conf, env, M=None):
    """``(M, ep_len, E)`` of one batch under ``conf``."""
    M = int(conf["timesteps_per_batch"] if M is None else M)
    ep_len = int(min(conf["max_timesteps_per_episode"], env.max_steps))
    return M, ep_len, -(-M // ep_len)


def draw_resets(env, E):
    """``[E, N+1, 2]`` start positions (predators, then the prey) from
    ``env.rng``, in the order of ``E`` calls of ``reset()``: the env's
    random stream is consumed as the host rollout consumes it."""
    out = np.empty((E, env.n + 1, 2))
    for e in range(E):
        out[e, : env.n] = env.rng.uniform(-1, 1, size=(env.n, 2))
        out[e, env.n] = env.rng.uniform(-1, 1, size=2)
    return out


def set_env_state(env, pred_pos, prey_pos, pred_vel=None, prey_vel=None):
    """Put ``env`` at the start of an episode in the given state
    (velocities default to rest, as after ``reset()``)."""
    env.t = 0
    env.pred_pos = np.array(pred_pos, dtype=float).reshape(env.n, 2)
    env.prey_pos = np.array(prey_pos, dtype=float).reshape(2)
    env.pred_vel = (
        np.zeros((env.n, 2)) if pred_vel is None
        else np.array(pred_vel, dtype=float).reshape(env.n, 2)
    )
    env.prey_vel = (
        np.zeros(2) if prey_vel is None
        else np.array(prey_vel, dtype=float).reshape(2)
    )


def state_from_obs(obs):
    """Inverse of ``SimpleTagEnv._observations``: ``(pred_pos, pred_vel,
    prey_pos, prey_vel)`` from the ``[N, obs_dim]`` observations of one
    step (each row holds the predator's own velocity and position, the
    prey's relative position and the prey's velocity)."""
    obs = np.asarray(obs, dtype=float)
    pred_vel, pred_pos = obs[:, 0:2].copy(), obs[:, 2:4].copy()
    prey_pos = pred_pos[0] + obs[0, -4:-2]
    prey_vel = obs[0, -2:].copy()
    return pred_pos, pred_vel, prey_pos, prey_vel


def gaussian_logp(eps, cov):
    """``MultivariateNormal(mean, cov*I).log_prob(mean + sqrt(cov)*eps)``
    for noise rows ``eps [..., A]``."""
    A = eps.shape[-1]
    return (
        -0.5 * (eps * eps).sum(dim=-1)
        - 0.5 * A * math.log(2 * math.pi * cov)
    )


def rollout_host_mirror(problem, resets, eps, M=None):
    """The kernel's rollout on the host: a real ``SimpleTagEnv`` set to
    ``resets[e]`` at the start of episode ``e``, the actor modules, and
    ``act = mean + sqrt(cov)*eps[e, t, i]``. Returns what
    ``DeviceRollout.run`` returns."""
    pr = problem
    conf = pr.conf
    N = pr.N
    M, ep_len, E = episode_shape(conf, pr.env, M)
    cov, gamma = float(conf["cov"]), float(conf["gamma"])
    dtype = next(pr.actors[0].parameters()).dtype
    env = copy.deepcopy(pr.env)
    resets = np.asarray(resets, dtype=float).reshape(E, N + 1, 2)
    obs_l = [[] for _ in range(N)]
    act_l = [[] for _ in range(N)]
    logp_l = [[] for _ in range(N)]
    rews, rtgs, ep_rew, last = [], [], [], []
    for e in range(E):
        set_env_state(env, resets[e, :N], resets[e, N])
        obs = env._observations()
        ep = []
        for t in range(min(ep_len, M - e * ep_len)):
            obs_t = torch.as_tensor(obs, dtype=dtype, device=pr.device)
            with torch.no_grad():
                acts = torch.stack([
                    pr.actors[i](obs_t[i])
                    + math.sqrt(cov) * eps[e, t, i].to(pr.device, dtype)
                    for i in range(N)
                ])
            lp = gaussian_logp(eps[e, t].to(pr.device, dtype), cov)
            obs, r, _, _ = env.step(acts.cpu().numpy())
            for i in range(N):
                obs_l[i].append(obs_t[i])
                act_l[i].append(acts[i])
                logp_l[i].append(lp[i])
            ep.append(float(r[0]))
        rews.extend(ep)
        ep_rew.append(float(sum(ep)))
        # what the last step() returned: the observation after the end
        last.append(torch.as_tensor(obs, dtype=dtype, device=pr.device))
        run, ep_rtgs = 0.0, []
        for r in reversed(ep):  # rollout()'s recursion
            run = r + gamma * run
            ep_rtgs.append(run)
        rtgs.extend(reversed(ep_rtgs))
    rtgs_t = torch.as_tensor(rtgs, dtype=dtype, device=pr.device)
    return dict(
        obs=torch.cat([torch.stack(o) for o in obs_l]),
        acts=torch.cat([torch.stack(a) for a in act_l]),
        logp=torch.cat([torch.stack(p) for p in logp_l]),
        rews=torch.as_tensor(rews, dtype=torch.float64, device=pr.device),
        rtgs=rtgs_t.repeat(N),
        ep_rew=torch.as_tensor(
            ep_rew, dtype=torch.float64, device=pr.device
        ),
        # [E, N, obs_dim] -> row l*E + e
        last_obs=torch.stack(last).transpose(0, 1).reshape(
            N * E, -1).contiguous(),
        M=M, ep_len=ep_len,
    )


class DeviceRollout:
    """Launches ``ext.ppo_rollout`` for a ``DistPPOProblem``. A problem
    outside the kernel's range is a ``ValueError`` here, never a host
    rollout."""

    def __init__(self, problem):
        _ = self.ext  # a missing extension fails here, not mid-round
        pr = problem
        self.pr = pr
        self.device = pr.device
        self.dtype = next(pr.actors[0].parameters()).dtype
        if self.dtype not in (torch.float32, torch.float64):
            raise ValueError("device rollout supports fp32/fp64 actors")
        env = pr.env
        if not 1 <= pr.N <= MAX_NODES:
            raise ValueError(
                f"device rollout supports at most {MAX_NODES} predators, "
                f"got {pr.N}"
            )
        if env.n_obst > MAX_OBSTACLES:
            raise ValueError(
                f"device rollout supports at most {MAX_OBSTACLES} "
                f"obstacles, got {env.n_obst}"
            )
        if env.act_dim != ACT_DIM:
            raise ValueError(
                f"device rollout needs action dim {ACT_DIM}, got "
                f"{env.act_dim}"
            )
        try:
            plan = shifted_plan(pr.actors[0], 0)
        except NotImplementedError as e:
            raise ValueError(f"device rollout: {e}") from e
        if len(plan) > MAX_LAYERS:
            raise ValueError(
                f"device rollout supports at most {MAX_LAYERS} layers"
            )
        for layer in plan:
            if layer.activation not in ("relu", "none"):
                raise ValueError(
                    "device rollout supports relu/none activations, got "
                    f"{layer.activation!r}"
                )
            if max(layer.in_dim, layer.out_dim) > MAX_WIDTH:
                raise ValueError(
                    f"device rollout supports layer widths <= {MAX_WIDTH}"
                    f", got {layer.in_dim}x{layer.out_dim}"
                )
        _, ep_len, _ = episode_shape(pr.conf, env)
        if not 1 <= ep_len <= MAX_EP_LEN:
            raise ValueError(
                f"device rollout supports episodes of 1..{MAX_EP_LEN} "
                f"steps, got {ep_len}"
            )
        self.N = pr.N
        self.obs_dim = env.obs_dim
        self._plan = (
            [layer.in_dim for layer in plan],
            [layer.out_dim for layer in plan],
            [layer.w_off for layer in plan],
            [layer.b_off for layer in plan],
            [ACT_IDS[layer.activation] for layer in plan],
        )
        self._envp = [
            env.pred_size, env.prey_size, env.obst_size, env.pred_accel,
            env.prey_accel, env.pred_max_speed, env.prey_max_speed,
            envs.DT, envs.DAMPING, envs.CONTACT_MARGIN, envs.CONTACT_FORCE,
        ]
        self._obst = torch.as_tensor(
            env.obst_pos, dtype=torch.float64
        ).reshape(-1, 2).to(self.device).contiguous()

    @property
    def ext(self):
        # looked up, not stored: the problem stays deep-copyable
        from ..ops import get_ext

        return get_ext()

    def shape(self, M=None):
        return episode_shape(self.pr.conf, self.pr.env, M)

    # ------------------------------------------------------------------
    def draw_resets(self, E):
        return draw_resets(self.pr.env, E)

    def draw_noise(self, E, ep_len=None):
        ep_len = self.shape()[1] if ep_len is None else ep_len
        return torch.randn(
            E, ep_len, self.N, ACT_DIM, device=self.device,
            dtype=self.dtype,
        )

    # ------------------------------------------------------------------
    def run(self, theta, resets=None, eps=None, M=None):
        """One batch of ``M`` steps with the actors of the ``[N, n]``
        stack ``theta``. Returns ``obs [N*M, obs_dim]``, ``acts [N*M,
        A]``, ``logp``/``rtgs [N*M]`` (engine dtype), ``rews [M]`` and
        ``ep_rew [E]`` (double), ``last_obs [N*E, obs_dim]`` (row ``l*E +
        e``: the observation after episode ``e``'s last step), plus ``M``
        and ``ep_len``."""
        M, ep_len, E = self.shape(M)
        N, dev, dt = self.N, self.device, self.dtype
        if theta.shape != (N, self.pr.n) or theta.dtype != dt:
            raise ValueError(
                f"theta must be the [{N}, {self.pr.n}] {dt} stack"
            )
        if resets is None:
            resets = self.draw_resets(E)
        if eps is None:
            eps = self.draw_noise(E, ep_len)
        resets = torch.as_tensor(
            np.asarray(resets), dtype=torch.float64
        ).reshape(E, N + 1, 2).to(dev).contiguous()
        eps = eps.to(dev, dt).reshape(E, ep_len, N, ACT_DIM).contiguous()

        def mk(*shape, dtype=dt):
            return torch.empty(*shape, device=dev, dtype=dtype)

        out = dict(
            obs=mk(N * M, self.obs_dim), acts=mk(N * M, ACT_DIM),
            logp=mk(N * M), rews=mk(M, dtype=torch.float64),
            rtgs=mk(N * M), ep_rew=mk(E, dtype=torch.float64),
            last_obs=mk(N * E, self.obs_dim), M=M, ep_len=ep_len,
        )
        conf = self.pr.conf
        self.ext.ppo_rollout(
            theta.contiguous(), *self._plan, resets, self._obst, eps,
            out["obs"], out["acts"], out["logp"], out["rews"],
            out["rtgs"], out["ep_rew"], M, ep_len, float(conf["cov"]),
            float(conf["gamma"]), self._envp, out["last_obs"],
        )
        return out
