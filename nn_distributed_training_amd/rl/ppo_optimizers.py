"""Decentralized PPO optimizers (DiNNO / DSGD / DSGT over actor+critic).

Algorithm parity with the reference's RL tree
(``RL/dist_rl/{dinno,dsgd,dsgt}PPO.py``): per communication round,
collect an on-policy rollout with every node's current actor, exchange
the concatenated [actor | critic] parameter vectors with graph
neighbors, and apply the respective decentralized update. Differences by
design:

* the actor and critic blocks live in ONE flat vector per node; dual
  ascent / mixing decompose per coordinate, so this is mathematically
  identical to the reference's twin-block bookkeeping while halving the
  bookkeeping code. DSGT's separate actor/critic step sizes
  (dsgtPPO.py:47-48) are kept via a per-coordinate alpha vector;
* the reference DSGDPPO's aliasing bugs (critic mix lists built from
  actors and written into the actor lists, dsgdPPO.py:21-23,:66-73) are
  NOT reproduced;
* mixing is snapshot-synchronous (same deviation as optimizers/dsgd.py,
  documented there).

Checkpoint layout parity (reference dinnoPPO.py:231-265): every
``save_freq`` iterations write ``trained/ppo_actors_tag_<alg>_<id>.pth``
/ ``ppo_critics_...``, plus ``avg_ep_rews_<alg>_<id>.npy``,
``timesteps_<alg>_<id>.npy`` and ``agreements_<alg>_<id>.npz``.
"""

from __future__ import annotations

import math
import os

import numpy as np
import torch


class _PPOBase:
    alg = "base"

    def __init__(self, problem, conf: dict):
        self.pr = problem
        self.conf = conf
        self.device = problem.device
        self.run_id = conf.get("run_id", "0")
        self.save_freq = conf.get("save_freq", 0)
        self.out_dir = conf.get("output_dir", "./trained")
        self.avg_ep_rews = []
        self.timesteps = []
        self.agreements_actor = []
        self.agreements_critic = []
        self.grad_engine = conf.get("grad_engine", "torch")
        self.engine = self._resolve_grad_engine()

    # ------------------------------------------------------------------
    def _resolve_grad_engine(self):
        """The StackedPPOEngine for ``grad_engine: "stacked"``, None for
        ``"torch"``. A stacked request that cannot be served is an
        error, never a quiet per-node run."""
        if self.grad_engine == "torch":
            return None
        if self.grad_engine != "stacked":
            raise ValueError(
                f"grad_engine must be 'torch' or 'stacked', got "
                f"{self.grad_engine!r}"
            )
        if self.device.type != "cuda":
            raise ValueError(
                "grad_engine='stacked' needs a GPU problem; this one is "
                f"on {self.device}"
            )
        from ..ops import get_ext

        try:
            get_ext()
        except Exception as e:  # noqa: BLE001
            raise ValueError(
                "grad_engine='stacked' needs the HIP extension, which "
                f"failed to load: {e}"
            ) from e
        from .stacked_ppo import StackedPPOEngine

        engine = StackedPPOEngine(self.pr)
        # rollout() takes V(obs) for the advantages from the engine
        self.pr.value_engine = engine
        return engine

    def _begin_round(self):
        """Hand the round's rollout to the stacked engine: a device
        rollout's [N*M, .] tensors as they are, a host rollout's
        per-node buffers concatenated."""
        if self.engine is None:
            return
        if self.pr.device_buf is not None:
            self.engine.load_device_rollout(self.pr.device_buf)
        else:
            self.engine.load_rollout(self.pr.buf)

    def _theta_stack(self):
        """[N, n] stack of the modules' current node vectors (a copy)."""
        pr = self.pr
        return torch.stack(
            [pr.node_vector(i).detach() for i in range(pr.N)]
        ).contiguous()

    def _grad_stack(self, theta):
        """[N, n] PPO gradients at the current parameters ``theta``.

        "torch": per-node autograd through the actor/critic modules,
        which the caller keeps equal to ``theta`` (a fresh tensor).
        "stacked": ``StackedPPOEngine.grads(theta)`` - no module, no
        autograd; the result is the engine's buffer, overwritten by the
        next call."""
        if self.engine is not None:
            return self.engine.grads(theta)
        pr = self.pr
        grads = []
        for i in range(pr.N):
            for p in pr.node_parameters(i):
                p.grad = None
            pred_loss = pr.local_batch_loss(i)
            pred_loss.backward()
            grads.append(
                torch.cat(
                    [
                        (p.grad if p.grad is not None
                         else torch.zeros_like(p)).reshape(-1)
                        for p in pr.node_parameters(i)
                    ]
                )
            )
        return torch.stack(grads).to(theta.dtype).contiguous()

    def _write_back(self, theta):
        """Load the stack rows into the actor/critic modules."""
        with torch.no_grad():
            for i in range(self.pr.N):
                self.pr.set_node_vector(i, theta[i].clone())

    def _snapshot_vectors(self):
        return {
            i: self.pr.node_vector(i).detach().clone()
            for i in range(self.pr.N)
        }

    def _neighbors(self, i):
        return list(self.pr.graph.neighbors(i))

    # ------------------------------------------------------------------
    def _record(self, it):
        self.avg_ep_rews.append(self.pr.ep_rew_history[-1])
        self.timesteps.append(self.pr.total_timesteps)
        aa, cc = self.pr.agreement()
        self.agreements_actor.append(aa.numpy())
        self.agreements_critic.append(cc.numpy())
        if self.conf.get("verbose", True):
            print(
                f"[{self.alg}] iter {it} t={self.pr.total_timesteps} "
                f"avg_ep_rew={self.avg_ep_rews[-1]:.2f} "
                f"agree_max={aa.max().item():.4f}",
                flush=True,
            )
        if self.save_freq and (it + 1) % self.save_freq == 0:
            self.save(it)

    def save(self, it=None):
        os.makedirs(self.out_dir, exist_ok=True)
        tag = f"tag_{self.alg}_{self.run_id}"
        if it is not None:
            tag_k = f"{tag}_{it + 1}"
        else:
            tag_k = tag
        torch.save(
            {i: self.pr.actors[i].state_dict()
             for i in range(self.pr.N)},
            os.path.join(self.out_dir, f"ppo_actors_{tag_k}.pth"),
        )
        torch.save(
            {i: self.pr.critics[i].state_dict()
             for i in range(self.pr.N)},
            os.path.join(self.out_dir, f"ppo_critics_{tag_k}.pth"),
        )
        np.save(
            os.path.join(self.out_dir, f"avg_ep_rews_{tag}.npy"),
            np.asarray(self.avg_ep_rews),
        )
        np.save(
            os.path.join(self.out_dir, f"timesteps_{tag}.npy"),
            np.asarray(self.timesteps),
        )
        np.savez(
            os.path.join(self.out_dir, f"agreements_{tag}.npz"),
            actor=np.stack(self.agreements_actor),
            critic=np.stack(self.agreements_critic),
        )

    # ------------------------------------------------------------------
    def train(self):
        max_t = self.conf.get("max_rl_timesteps", 10_000)
        it = 0
        while self.pr.total_timesteps < max_t:
            self.pr.rollout()
            self.step_round(it)
            self._record(it)
            it += 1
        self.save()


class DiNNOPPO(_PPOBase):
    """Consensus-ADMM PPO (reference dinnoPPO.py:6-269)."""

    alg = "cadmm"

    def __init__(self, problem, conf):
        super().__init__(problem, conf)
        self.rho = conf.get("rho_init", 0.3)
        self.rho_scaling = conf.get("rho_scaling", 1.0)
        self.pits = conf.get("primal_iterations", 5)
        oits = conf.get("expected_iterations", 200)
        lr0 = conf.get("primal_lr_start", 1e-3)
        lr1 = conf.get("primal_lr_finish", 1e-4)
        decay = conf.get("lr_decay_type", "log")
        if decay == "constant":
            self.lr = lr0 * torch.ones(oits)
        elif decay == "linear":
            self.lr = torch.linspace(lr0, lr1, oits)
        else:
            self.lr = torch.logspace(
                math.log10(lr0), math.log10(lr1), oits
            )
        self.duals = {
            i: torch.zeros(problem.n, device=self.device)
            for i in range(problem.N)
        }

    # ------------------------------------------------------------------
    def _hip_available(self):
        if os.environ.get("NDTA_RL_HIP", "1") == "0":
            return False
        if self.device.type != "cuda":
            return False
        from ..ops import ext_available

        return ext_available()

    def _csr(self):
        """CSR neighbor tables over all nodes (single-process RL)."""
        if getattr(self, "_csr_cache", None) is None:
            offs, idx = [0], []
            for i in range(self.pr.N):
                ns = self._neighbors(i)
                idx.extend(ns)
                offs.append(len(idx))
            dev = self.device
            self._csr_cache = (
                torch.tensor(offs, dtype=torch.int32, device=dev),
                torch.tensor(idx, dtype=torch.int32, device=dev),
                torch.tensor(
                    [len(self._neighbors(i)) for i in range(self.pr.N)],
                    dtype=torch.int32, device=dev,
                ),
            )
        return self._csr_cache

    def _step_round_hip(self, it, lr):
        """DiNNO round math on the stacked CDNA4 kernels (VERDICT r1
        item 9; reference round math RL/dist_rl/dinnoPPO.py:87-131):
        the [actor|critic] vectors of all nodes form one [N, n] stack;
        dual ascent + s-reduction run in ONE dinno_dual_threg launch
        and each primal step is ONE fused penalty-Adam launch (the
        analytic consensus-penalty gradient folds into the update).
        The pred-loss gradient comes from ``_grad_stack``. With
        ``grad_engine: "torch"`` it is per-node autograd, and theta is
        copied back into the modules after every primal step so the
        next autograd sees it. With ``"stacked"`` it is
        ``StackedPPOEngine.grads``: theta stays on the device for all
        primal iterations (grads, fused_step, nothing in between) and
        reaches the modules once, at the end of the round. The rollout is
        the problem's: host-side env stepping, or with ``rollout_engine:
        "device"`` one kernel launch whose tensors the stacked engine
        adopts without a copy (``_begin_round``)."""
        from ..ops import get_ext

        ext = get_ext()
        pr = self.pr
        self._begin_round()
        ths = self._theta_stack()
        if getattr(self, "_duals_t", None) is None:
            self._duals_t = torch.zeros_like(ths)
            self._s_t = torch.empty_like(ths)
            self._m_t = torch.empty_like(ths)
            self._v_t = torch.empty_like(ths)
        offs, idx, deg = self._csr()
        ext.dinno_dual_threg(
            ths, None, offs, idx, self._duals_t, self._s_t, self.rho
        )
        # dict view kept in sync for checkpoints/inspection
        for i in range(pr.N):
            self.duals[i] = self._duals_t[i]
        theta = ths.clone()
        for pit in range(self.pits):
            grad = self._grad_stack(theta)
            # fresh Adam per round (reference recreates the optimizer):
            # first_step resets the moments, step_t restarts at 1
            ext.fused_step(
                theta, grad, self._duals_t, self._s_t, deg,
                self._m_t, self._v_t,
                self.rho, lr, 0.9, 0.999, 1e-8, 0.0,
                pit + 1, 0, pit == 0, 1, False,
            )
            if self.engine is None:
                for i in range(pr.N):
                    pr.set_node_vector(i, theta[i])
        if self.engine is not None:
            self._write_back(theta)

    def step_round(self, it):
        pr = self.pr
        self.rho *= self.rho_scaling
        lr = float(self.lr[min(it, len(self.lr) - 1)])
        if self.engine is not None or self._hip_available():
            return self._step_round_hip(it, lr)
        ths = self._snapshot_vectors()
        for i in range(pr.N):
            neighs = self._neighbors(i)
            thj = torch.stack([ths[j] for j in neighs])
            self.duals[i] += self.rho * torch.sum(ths[i] - thj, dim=0)
            th_reg = 0.5 * (thj + ths[i])
            opt = torch.optim.Adam(pr.node_parameters(i), lr)
            for _ in range(self.pits):
                opt.zero_grad()
                pred_loss = pr.local_batch_loss(i)
                th = pr.node_vector(i)
                reg = torch.sum(
                    torch.square(th.unsqueeze(0) - th_reg)
                )
                loss = (
                    pred_loss
                    + torch.dot(th, self.duals[i])
                    + self.rho * reg
                )
                loss.backward()
                opt.step()


class DSGDPPO(_PPOBase):
    """Decentralized SGD PPO (reference dsgdPPO.py:7-165, minus its
    actor/critic aliasing bugs)."""

    alg = "dsgd"

    def __init__(self, problem, conf):
        super().__init__(problem, conf)
        self.alph = conf.get("alpha0", 1e-3)
        self.mu = conf.get("mu", 1e-3)

    def step_round(self, it):
        from ..utils import graph_generation

        pr = self.pr
        W = graph_generation.get_metropolis(pr.graph).to(self.device)
        self.alph = self.alph * (1 - self.mu * self.alph)
        self._begin_round()
        ths = self._snapshot_vectors()
        rows = []
        for i in range(pr.N):
            mixed = W[i, i] * ths[i]
            for j in self._neighbors(i):
                mixed = mixed + W[i, j] * ths[j]
            if self.engine is None:
                pr.set_node_vector(i, mixed)
            rows.append(mixed)
        theta = torch.stack(rows).contiguous()
        grad = self._grad_stack(theta)
        self._write_back(theta.add(grad, alpha=-self.alph))


class DSGTPPO(_PPOBase):
    """Gradient-tracking PPO (reference dsgtPPO.py:7-254) with separate
    actor/critic step sizes kept as a per-coordinate alpha vector."""

    alg = "dsgt"

    def __init__(self, problem, conf):
        super().__init__(problem, conf)
        a_act = conf.get("alpha_actor", 1e-3)
        a_cri = conf.get("alpha_critic", conf.get("alpha_actor", 1e-3))
        self.alpha_vec = torch.cat(
            [
                torch.full((problem.n_actor,), a_act),
                torch.full((problem.n_critic,), a_cri),
            ]
        ).to(self.device)
        self.y = {
            i: torch.zeros(problem.n, device=self.device)
            for i in range(problem.N)
        }
        self.g = {
            i: torch.zeros(problem.n, device=self.device)
            for i in range(problem.N)
        }
        self._bootstrapped = False

    def step_round(self, it):
        from ..utils import graph_generation

        pr = self.pr
        self._begin_round()
        if not self._bootstrapped:
            # reference dsgtPPO.py:58-85 bootstraps y, g from the
            # first rollout's gradients
            grad = self._grad_stack(self._theta_stack())
            for i in range(pr.N):
                self.y[i] = grad[i].clone()
                self.g[i] = grad[i].clone()
            self._bootstrapped = True

        W = graph_generation.get_metropolis(pr.graph).to(self.device)
        ths = self._snapshot_vectors()
        ys = {i: self.y[i].clone() for i in range(pr.N)}
        y_new = {}
        rows = []
        for i in range(pr.N):
            p_mix = W[i, i] * (ths[i] - self.alpha_vec * ys[i])
            y_mix = W[i, i] * ys[i]
            for j in self._neighbors(i):
                p_mix = p_mix + W[i, j] * (
                    ths[j] - self.alpha_vec * ys[j]
                )
                y_mix = y_mix + W[i, j] * ys[j]
            rows.append(p_mix)
            y_new[i] = y_mix
        theta = torch.stack(rows).contiguous()
        # the mixed parameters are the round's result; "torch" needs
        # them in the modules before its autograd as well
        self._write_back(theta)
        grad = self._grad_stack(theta)
        for i in range(pr.N):
            g_next = grad[i].clone()
            self.y[i] = y_new[i] + g_next - self.g[i]
            self.g[i] = g_next


def build_ppo_optimizer(alg, problem, conf):
    cls = {"dinno": DiNNOPPO, "cadmm": DiNNOPPO, "dsgd": DSGDPPO,
           "dsgt": DSGTPPO}[alg]
    return cls(problem, conf)
