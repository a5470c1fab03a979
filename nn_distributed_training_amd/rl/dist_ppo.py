"""Distributed multi-agent PPO problem (predator-prey tag).

Capability parity with the reference's ``RL/dist_rl/dist_ppo.py``: N
predators = N graph nodes, each holding an actor+critic pair; rollouts
step ONE shared environment with every node's current actor; rewards-to-
go, advantage normalization, clipped-surrogate + MSE-critic loss, and
Gaussian action sampling with a fixed covariance (cov 0.5, reference
dist_ppo.py:325-351). Hyperparameters come from a plain config dict (the
reference's ``exec``-based injection, dist_ppo.py:426-427, is not
reproduced).

``rollout_engine: "device"`` (default ``"host"``) collects the batch and
runs ``evaluate`` in one kernel launch instead (rl/device_rollout.py);
its action noise comes from another random stream than
``MultivariateNormal.sample``'s.

``gae_lambda`` (default ``None``: the reference's Monte-Carlo estimator
above) switches the advantages to GAE(lambda) (rl/advantages.py), and
``critic_target: "lambda"`` (default ``"rtg"``) then regresses the critic
on the lambda-returns instead of the rewards-to-go.

``bootstrap_truncated`` (default ``False``: an episode's end counts as
terminal, as in the reference) treats every episode end as what it is in
this env, a time-limit truncation, and continues the return beyond it
with ``gamma * V(o')``, the critic's value of the observation the env
returned after the episode's last step (partial-episode bootstrapping,
Pardo et al. 2018; rl/advantages.py has the formulas). The rewards-to-go,
the advantages of either estimator and the lambda-returns all carry the
tail; ``last_obs`` keeps those observations. It is an addition the
reference does not have and consumes no randomness.
"""

from __future__ import annotations

import copy

import numpy as np
import torch
from torch.distributions import MultivariateNormal

from ..models.mlp import FFReLUNet
from .envs import SimpleTagEnv

DEFAULTS = dict(
    timesteps_per_batch=600,
    max_timesteps_per_episode=100,
    gamma=0.99,
    clip=0.2,
    critic_coef=0.5,
    cov=0.5,
    hidden=(64, 64, 64),
)


class DistPPOProblem:
    def __init__(self, graph, env: SimpleTagEnv, device, conf: dict):
        self.graph = graph
        self.env = env
        self.device = torch.device(device)
        self.conf = {**DEFAULTS, **conf}

        self.N = graph.number_of_nodes()
        assert self.N == env.n, "one predator per graph node"

        obs_dim, act_dim = env.obs_dim, env.act_dim
        hid = list(self.conf["hidden"])
        base_actor = FFReLUNet([obs_dim, *hid, act_dim])
        base_critic = FFReLUNet([obs_dim, *hid, 1])
        self.actors = {
            i: copy.deepcopy(base_actor).to(self.device)
            for i in range(self.N)
        }
        self.critics = {
            i: copy.deepcopy(base_critic).to(self.device)
            for i in range(self.N)
        }
        self.n_actor = sum(p.numel() for p in base_actor.parameters())
        self.n_critic = sum(p.numel() for p in base_critic.parameters())
        self.n = self.n_actor + self.n_critic

        cov = self.conf["cov"]
        self.cov_mat = torch.eye(act_dim, device=self.device) * cov

        # rollout buffers (per node), populated by rollout()
        self.buf = None
        # optional hook: an engine with load_obs()/values() (the
        # optimizers' grad_engine="stacked" attaches its
        # StackedPPOEngine); rollout() then takes V(obs) from it
        self.value_engine = None
        self.total_timesteps = 0
        self.ep_rew_history = []  # mean episodic reward per batch
        # rollout_engine "device": the DeviceRollout, and the [N*M, .]
        # tensors of its last batch (self.buf then holds views of them)
        self.rollout_engine = self.conf.get("rollout_engine", "host")
        self.device_rollout = self._resolve_rollout_engine()
        self.device_buf = None
        (self.gae_lambda, self.critic_target,
         self.bootstrap_truncated) = self._resolve_estimator()
        # [N*E, obs_dim], row l*E + e: node l's observation after the
        # last step of episode e of the latest rollout()
        self.last_obs = None

    # ------------------------------------------------------------------
    def _resolve_estimator(self):
        """``(gae_lambda, critic_target, bootstrap_truncated)`` of the
        config, checked."""
        lam = self.conf.get("gae_lambda")
        target = self.conf.get("critic_target", "rtg")
        boot = self.conf.get("bootstrap_truncated", False)
        if lam is not None:
            lam = float(lam)
            if not 0.0 <= lam <= 1.0:
                raise ValueError(
                    f"gae_lambda must be in [0, 1] or None, got {lam}"
                )
        if target not in ("rtg", "lambda"):
            raise ValueError(
                f"critic_target must be 'rtg' or 'lambda', got {target!r}"
            )
        if target == "lambda" and lam is None:
            raise ValueError(
                "critic_target='lambda' needs a gae_lambda: the "
                "lambda-returns come from the GAE estimator"
            )
        if not isinstance(boot, bool):
            raise ValueError(
                f"bootstrap_truncated must be True or False, got {boot!r}"
            )
        return lam, target, boot

    def _gae(self, v, rews, ep_lens, v_last=None):
        """GAE(lambda) from the critic values ``v [N, M]`` and the
        rewards (``[M]`` shared or ``[N, M]``, double): the normalised
        advantages and the critic target (None under ``"rtg"``), both
        ``[N, M]`` of ``v``'s dtype. ``v_last [N, E]`` bootstraps the
        episodes' ends (None: terminal). One ``ppo_gae`` launch where the
        extension is guaranteed (device rollout or stacked engine) and
        the episodes are uniform, the torch mirror otherwise."""
        from . import advantages as gae

        gamma, lam = float(self.conf["gamma"]), self.gae_lambda
        want_ret = self.critic_target == "lambda"
        ep_len = gae.uniform_ep_len(ep_lens)
        have_ext = (
            self.device_rollout is not None
            or self.value_engine is not None
        )
        if have_ext and ep_len is not None:
            return gae.gae_advantages_hip(
                v, rews, ep_len, gamma, lam, want_ret, v_last
            )
        A, ret = gae.gae_advantages_torch(
            v, rews, ep_lens, gamma, lam, v_last
        )
        adv = gae.normalize_advantages(A).to(v.dtype)
        return adv, ret.to(v.dtype) if want_ret else None

    def _values_last(self, theta=None):
        """``V_end [N, E]``: every node's critic on its rows of
        ``self.last_obs``, with the parameters that give ``V(obs)`` for
        the batch - the stacked engine's forward at ``theta`` (default:
        the modules' parameters) where one is attached, else the critic
        modules."""
        N = self.N
        if self.value_engine is not None:
            eng = self.value_engine
            if theta is None:
                theta = eng.stack_from_modules()
            return eng.values_last(theta, self.last_obs)
        E = self.last_obs.shape[0] // N
        with torch.no_grad():
            return torch.stack([
                self.critics[i](self.last_obs[i * E:(i + 1) * E])
                .squeeze(-1)
                for i in range(N)
            ])

    def _node_mc_adv(self, i):
        """Node ``i``'s normalised Monte-Carlo advantages ``rtg - V(obs)``
        from its critic module."""
        b = self.buf[i]
        with torch.no_grad():
            v = self.critics[i](b["obs"]).squeeze(-1)
        adv = b["rtgs"] - v
        return (adv - adv.mean()) / (adv.std() + 1e-10)

    # ------------------------------------------------------------------
    def _resolve_rollout_engine(self):
        """The DeviceRollout for ``rollout_engine: "device"``, None for
        ``"host"``. A device request that cannot be served is an error,
        never a quiet host rollout."""
        if self.rollout_engine == "host":
            return None
        if self.rollout_engine != "device":
            raise ValueError(
                f"rollout_engine must be 'host' or 'device', got "
                f"{self.rollout_engine!r}"
            )
        if self.device.type != "cuda":
            raise ValueError(
                "rollout_engine='device' needs a GPU problem; this one "
                f"is on {self.device}"
            )
        from ..ops import get_ext

        try:
            get_ext()
        except Exception as e:  # noqa: BLE001
            raise ValueError(
                "rollout_engine='device' needs the HIP extension, which "
                f"failed to load: {e}"
            ) from e
        from .device_rollout import DeviceRollout

        return DeviceRollout(self)

    # ------------------------------------------------------------------
    def node_vector(self, i) -> torch.Tensor:
        """Concatenated [actor | critic] flat parameters of node i."""
        return torch.cat(
            [
                torch.nn.utils.parameters_to_vector(
                    self.actors[i].parameters()
                ),
                torch.nn.utils.parameters_to_vector(
                    self.critics[i].parameters()
                ),
            ]
        )

    def set_node_vector(self, i, vec: torch.Tensor):
        torch.nn.utils.vector_to_parameters(
            vec[: self.n_actor], self.actors[i].parameters()
        )
        torch.nn.utils.vector_to_parameters(
            vec[self.n_actor :], self.critics[i].parameters()
        )

    def node_parameters(self, i):
        return list(self.actors[i].parameters()) + list(
            self.critics[i].parameters()
        )

    # ------------------------------------------------------------------
    def get_action(self, i, obs_t: torch.Tensor):
        mean = self.actors[i](obs_t)
        dist = MultivariateNormal(mean, self.cov_mat)
        act = dist.sample()
        return act, dist.log_prob(act)

    # ------------------------------------------------------------------
    def rollout(self):
        """Collect one on-policy batch by stepping the shared env.

        Parity with reference split_rollout_marl (dist_ppo.py:171-293):
        serial env stepping, per-predator trajectories, rewards-to-go,
        advantage = rtg - V(obs) normalized per node. ``buf[i]["rews"]``
        keeps the per-step rewards (double). With ``gae_lambda`` the
        advantages are GAE(lambda) instead (``_finish_gae``), and
        ``critic_target: "lambda"`` adds the lambda-returns as
        ``buf[i]["vtarg"]``. With ``bootstrap_truncated`` the rewards-to-
        go, and through them or through ``_gae`` the advantages and the
        lambda-returns, go on beyond every episode's end with the
        critic's value of ``last_obs``.
        """
        if self.device_rollout is not None:
            return self._rollout_device()
        conf = self.conf
        T = conf["timesteps_per_batch"]
        obs_buf = [[] for _ in range(self.N)]
        act_buf = [[] for _ in range(self.N)]
        logp_buf = [[] for _ in range(self.N)]
        rews_eps = [[] for _ in range(self.N)]  # list of per-ep lists
        ep_total_rews = []
        ep_last_obs = []  # per episode: what its last step() returned

        t = 0
        while t < T:
            obs = self.env.reset()
            ep_rews = [[] for _ in range(self.N)]
            for _ in range(conf["max_timesteps_per_episode"]):
                t += 1
                obs_t = torch.as_tensor(
                    obs, dtype=torch.get_default_dtype(),
                    device=self.device,
                )
                acts, logps = [], []
                with torch.no_grad():
                    for i in range(self.N):
                        a, lp = self.get_action(i, obs_t[i])
                        acts.append(a)
                        logps.append(lp)
                a_np = torch.stack(acts).cpu().numpy()
                nobs, rews, done, _ = self.env.step(a_np)
                for i in range(self.N):
                    obs_buf[i].append(obs_t[i])
                    act_buf[i].append(acts[i])
                    logp_buf[i].append(logps[i])
                    ep_rews[i].append(float(rews[i]))
                obs = nobs
                if done or t >= T:
                    break
            for i in range(self.N):
                rews_eps[i].append(ep_rews[i])
            ep_last_obs.append(nobs)
            ep_total_rews.append(
                float(np.mean([sum(r) for r in ep_rews]))
            )

        self.total_timesteps += t
        self.ep_rew_history.append(float(np.mean(ep_total_rews)))
        # [E, N, obs_dim] -> row l*E + e
        self.last_obs = torch.as_tensor(
            np.stack(ep_last_obs).swapaxes(0, 1).reshape(
                self.N * len(ep_last_obs), -1),
            dtype=torch.get_default_dtype(), device=self.device,
        )
        ep_lens = [len(ep) for ep in rews_eps[0]]
        boot = self.bootstrap_truncated

        gamma = conf["gamma"]
        self.buf = {}
        for i in range(self.N):
            rtgs = []
            for ep in rews_eps[i]:
                run = 0.0
                ep_rtgs = []
                for r in reversed(ep):
                    run = r + gamma * run
                    ep_rtgs.append(run)
                rtgs.extend(reversed(ep_rtgs))
            obs_i = torch.stack(obs_buf[i])
            acts_i = torch.stack(act_buf[i])
            logp_i = torch.stack(logp_buf[i])
            rtgs_i = torch.as_tensor(
                rtgs, dtype=torch.get_default_dtype(),
                device=self.device,
            )
            rews_i = torch.as_tensor(
                [r for ep in rews_eps[i] for r in ep],
                dtype=torch.float64, device=self.device,
            )
            self.buf[i] = dict(
                obs=obs_i, acts=acts_i, logp=logp_i, rtgs=rtgs_i,
                rews=rews_i,
            )
            if self.gae_lambda is not None or boot:
                continue
            if self.value_engine is None:
                self.buf[i]["adv"] = self._node_mc_adv(i)
        v_last = None
        if boot:
            from .advantages import bootstrap_rtgs

            v_last = self._values_last()
            rtgs_b = bootstrap_rtgs(
                torch.stack([self.buf[i]["rtgs"] for i in range(self.N)]),
                v_last, ep_lens, gamma,
            )
            for i in range(self.N):
                self.buf[i]["rtgs"] = rtgs_b[i]
        if self.gae_lambda is not None:
            self._finish_gae(ep_lens, v_last)
        elif boot and self.value_engine is None:
            for i in range(self.N):
                self.buf[i]["adv"] = self._node_mc_adv(i)
        elif self.value_engine is not None:
            # V(obs) of all nodes from the stacked critic forward, then
            # the same per-node normalization batched over [N, M]
            eng = self.value_engine
            eng.load_obs([self.buf[i]["obs"] for i in range(self.N)])
            v = eng.values(eng.stack_from_modules())
            adv = torch.stack(
                [self.buf[i]["rtgs"] for i in range(self.N)]
            ) - v
            adv = (adv - adv.mean(dim=1, keepdim=True)) / (
                adv.std(dim=1, keepdim=True) + 1e-10
            )
            for i in range(self.N):
                self.buf[i]["adv"] = adv[i]

    def _finish_gae(self, ep_lens, v_last=None):
        """``adv`` (and ``vtarg``) of a host rollout's buffers under
        ``gae_lambda``: V(obs) from the stacked engine where one is
        attached, else from the critic modules. ``v_last``: see
        :meth:`_gae`."""
        N = self.N
        if self.value_engine is None:
            with torch.no_grad():
                v = torch.stack([
                    self.critics[i](self.buf[i]["obs"]).squeeze(-1)
                    for i in range(N)
                ])
        else:
            eng = self.value_engine
            eng.load_obs([self.buf[i]["obs"] for i in range(N)])
            v = eng.values(eng.stack_from_modules())
        rews = torch.stack([self.buf[i]["rews"] for i in range(N)])
        adv, vtarg = self._gae(v, rews, ep_lens, v_last)
        for i in range(N):
            self.buf[i]["adv"] = adv[i]
            if vtarg is not None:
                self.buf[i]["vtarg"] = vtarg[i]

    # ------------------------------------------------------------------
    def _theta_stack(self):
        return torch.stack(
            [self.node_vector(i).detach() for i in range(self.N)]
        ).contiguous()

    def _rollout_device(self):
        """The same batch from one ``ext.ppo_rollout`` launch
        (rl/device_rollout.py): ``self.buf[i]`` are views of the
        ``[N*M, .]`` tensors kept in ``self.device_buf``."""
        N = self.N
        theta = self._theta_stack()
        out = self.device_rollout.run(theta)
        M = out["M"]
        self.total_timesteps += M
        self.ep_rew_history.append(float(out["ep_rew"].mean()))
        self.last_obs = out["last_obs"]
        ep_len = out["ep_len"]
        ep_lens = [min(ep_len, M - s) for s in range(0, M, ep_len)]

        rtgs = out["rtgs"].view(N, M)
        if self.value_engine is None:
            with torch.no_grad():
                v = torch.stack([
                    self.critics[i](out["obs"][i * M:(i + 1) * M])
                    .squeeze(-1)
                    for i in range(N)
                ])
        else:
            eng = self.value_engine
            eng.load_device_rollout(out)
            v = eng.values(theta)
        v_last = None
        if self.bootstrap_truncated:
            from .advantages import bootstrap_rtgs

            v_last = self._values_last(theta)
            # in place: out["rtgs"] stays the tensor the engine adopted
            rtgs.copy_(bootstrap_rtgs(
                rtgs, v_last, ep_lens, float(self.conf["gamma"])
            ))
        keys = ["obs", "acts", "logp", "rtgs", "adv"]
        if self.gae_lambda is not None:
            adv, vtarg = self._gae(v, out["rews"], ep_lens, v_last)
            if vtarg is not None:
                out["vtarg"] = vtarg.reshape(-1)
                keys.append("vtarg")
        else:
            adv = rtgs - v
            adv = (adv - adv.mean(dim=1, keepdim=True)) / (
                adv.std(dim=1, keepdim=True) + 1e-10
            )
        out["adv"] = adv.reshape(-1)
        self.device_buf = out
        self.buf = {
            i: {k: out[k][i * M:(i + 1) * M] for k in keys}
            for i in range(N)
        }
        for i in range(N):
            self.buf[i]["rews"] = out["rews"]  # one team reward row

    # ------------------------------------------------------------------
    def local_batch_loss(self, i):
        """Clipped PPO surrogate + critic MSE on node i's rollout
        (reference ev_ppo_loss, dist_ppo.py:128-156)."""
        b = self.buf[i]
        mean = self.actors[i](b["obs"])
        dist = MultivariateNormal(mean, self.cov_mat)
        logp = dist.log_prob(b["acts"])
        ratios = torch.exp(logp - b["logp"])
        clip = self.conf["clip"]
        s1 = ratios * b["adv"]
        s2 = torch.clamp(ratios, 1 - clip, 1 + clip) * b["adv"]
        actor_loss = -torch.min(s1, s2).mean()
        v = self.critics[i](b["obs"]).squeeze(-1)
        # critic_target "lambda" carries the lambda-returns as "vtarg"
        critic_loss = torch.nn.functional.mse_loss(
            v, b.get("vtarg", b["rtgs"])
        )
        return actor_loss + self.conf["critic_coef"] * critic_loss

    # ------------------------------------------------------------------
    def agreement(self):
        """Normalized pairwise parameter distances (actor, critic)."""
        with torch.no_grad():
            av = torch.stack(
                [
                    torch.nn.utils.parameters_to_vector(
                        self.actors[i].parameters()
                    )
                    for i in range(self.N)
                ]
            )
            cv = torch.stack(
                [
                    torch.nn.utils.parameters_to_vector(
                        self.critics[i].parameters()
                    )
                    for i in range(self.N)
                ]
            )
            an = torch.nn.functional.normalize(av, dim=1)
            cn = torch.nn.functional.normalize(cv, dim=1)
            return (
                torch.cdist(an, an).cpu(),
                torch.cdist(cn, cn).cpu(),
            )

    # ------------------------------------------------------------------
    def evaluate(self, episodes=3):
        """Mean episodic reward with deterministic (mean) actions."""
        if self.device_rollout is not None:
            # the rollout kernel with zero noise: act = mean
            dr = self.device_rollout
            _, ep_len, _ = dr.shape()
            eps = torch.zeros(
                episodes, ep_len, self.N, self.env.act_dim,
                device=self.device, dtype=dr.dtype,
            )
            out = dr.run(
                self._theta_stack(), eps=eps, M=episodes * ep_len
            )
            return float(out["ep_rew"].mean())
        totals = []
        for _ in range(episodes):
            obs = self.env.reset()
            tot = 0.0
            for _ in range(self.conf["max_timesteps_per_episode"]):
                obs_t = torch.as_tensor(
                    obs, dtype=torch.get_default_dtype(),
                    device=self.device,
                )
                with torch.no_grad():
                    a = torch.stack(
                        [
                            self.actors[i](obs_t[i])
                            for i in range(self.N)
                        ]
                    )
                obs, rews, done, _ = self.env.step(a.cpu().numpy())
                tot += float(np.mean(rews))
                if done:
                    break
            totals.append(tot)
        return float(np.mean(totals))
