"""Batched PPO gradients on the stacked HIP kernels.

The per-node autograd of ``DistPPOProblem.local_batch_loss`` (a
``MultivariateNormal`` plus eager backward through two MLPs, once per
node) becomes a fixed sequence of launches for ALL nodes: every node's
``[actor | critic]`` vector is one row of a ``[N, n]`` stack (the order of
``DistPPOProblem.node_vector``), both nets run through the stacked
linear kernels, and ``ext.ppo_loss_bwd`` (ops/hip/losses.hip) turns the
two nets' outputs into the gradients with respect to them.

:func:`ppo_loss_grads_torch` is the kernel's formula in plain torch: the
documentation of what the kernel computes and the oracle of the CPU
tests.
"""

from __future__ import annotations

import dataclasses
import math

import torch

from ..models.spec import model_spec
from ..ops.stacked import ACT_IDS


def ppo_loss_grads_torch(mean, acts, old_logp, adv, v, rtgs, M, cov,
                         clip, critic_coef, loss_scale=1.0):
    """Mirror of ``ppo_loss_bwd_k``: ``(dmean, dv, loss)``.

    ``mean``/``acts`` are ``[L*M, A]``, the other inputs ``[L*M]``; node
    ``l`` owns rows ``[l*M, (l+1)*M)`` and every mean is over one node's
    ``M`` rows. ``loss`` is ``[L, 2]``: (actor term, critic term), so a
    node's objective is ``loss[l, 0] + critic_coef * loss[l, 1]``.
    """
    A = mean.shape[1]
    lo, hi = 1 - clip, 1 + clip
    d = acts - mean
    logp = (
        -0.5 * (d * d).sum(dim=1) / cov
        - 0.5 * A * math.log(2 * math.pi * cov)
    )
    r = torch.exp(logp - old_logp)
    s1 = r * adv
    s2 = torch.clamp(r, lo, hi) * adv
    # subgradient of min(s1, s2) w.r.t. r under torch's conventions:
    # clamp passes the gradient on [lo, hi] inclusive, and minimum
    # splits a tie evenly between two branches that then both carry adv
    passes = (
        ((r >= lo) & (r <= hi))
        | ((adv > 0) & (r < lo))
        | ((adv < 0) & (r > hi))
    )
    g = torch.where(passes, adv, torch.zeros_like(adv))
    dmean = -loss_scale * (g * r / cov / M).unsqueeze(1) * d
    e = v - rtgs
    dv = loss_scale * critic_coef * 2 * e / M
    loss = torch.stack(
        [
            -torch.minimum(s1, s2).reshape(-1, M).mean(dim=1),
            (e * e).reshape(-1, M).mean(dim=1),
        ],
        dim=1,
    )
    return dmean, dv, loss


def shifted_plan(model, shift):
    """``model_spec(model)``'s layers with ``w_off``/``b_off`` moved by
    ``shift`` elements: the plan of a net that starts ``shift`` elements
    into a longer flat vector."""
    plan = []
    for layer in model_spec(model).layers:
        if layer.kind != "linear" or layer.activation not in ACT_IDS:
            raise NotImplementedError(
                f"stacked PPO engine: unsupported layer {layer}"
            )
        plan.append(
            dataclasses.replace(
                layer, w_off=layer.w_off + shift, b_off=layer.b_off + shift
            )
        )
    if plan[-1].activation != "none":
        raise NotImplementedError(
            "stacked PPO engine needs a linear output layer"
        )
    return plan


class StackedPPOEngine:
    """Gradients of every node's PPO objective in a fixed number of
    launches: actor forward, critic forward, ``ppo_loss_bwd``, actor
    backward, critic backward. ``grads`` and ``values`` touch no
    ``nn.Module`` and no autograd; the optimizers write the stack back
    to the modules once per round (``set_node_vector``)."""

    def __init__(self, problem):
        _ = self.ext  # a missing extension fails here, not mid-round
        self.pr = problem
        self.device = problem.device
        self.dtype = torch.get_default_dtype()
        if self.dtype not in (torch.float32, torch.float64):
            raise ValueError("stacked PPO engine supports fp32/fp64")
        self.N = problem.N
        self.n = problem.n
        self.actor_plan = shifted_plan(problem.actors[0], 0)
        self.critic_plan = shifted_plan(
            problem.critics[0], problem.n_actor
        )
        self.A = self.actor_plan[-1].out_dim
        assert self.critic_plan[-1].out_dim == 1
        self.theta = self.stack_from_modules()
        self.grad = torch.zeros_like(self.theta)
        self.M = None
        # values_last()'s own activation rows, by E
        self._last_bufs = {}
        self._loss = torch.zeros(
            self.N, 2, device=self.device, dtype=self.dtype
        )

    @property
    def ext(self):
        # looked up, not stored: the problem that carries this engine
        # as its value hook stays deep-copyable
        from ..ops import get_ext

        return get_ext()

    # ------------------------------------------------------------------
    def stack_from_modules(self):
        """Fresh ``[N, n]`` stack of the modules' current parameters."""
        pr = self.pr
        return torch.stack(
            [
                pr.node_vector(i).detach().to(self.device, self.dtype)
                for i in range(pr.N)
            ]
        ).contiguous()

    # ------------------------------------------------------------------
    def _alloc(self, M):
        rows = self.N * M

        def mk(el):
            return torch.empty(
                rows, el, device=self.device, dtype=self.dtype
            )

        def pack(plan):
            return {
                "acts": [mk(layer.out_dim) for layer in plan],
                "dzs": [mk(layer.out_dim) for layer in plan],
            }

        self.M = M
        self._actor_bufs = pack(self.actor_plan)
        self._critic_bufs = pack(self.critic_plan)
        # True when a dW kernel of either net adds into the grad stack
        self._zero_grad = any(
            self.ext.dw_accumulates(M, layer.in_dim, layer.out_dim)
            for layer in self.actor_plan + self.critic_plan
        )

    def load_rollout(self, buf):
        """Stack ``DistPPOProblem.buf`` into ``[N*M, .]`` tensors."""
        Ms = {int(buf[i]["obs"].shape[0]) for i in range(self.N)}
        assert len(Ms) == 1, f"nodes differ in rollout length: {Ms}"
        self.load_obs([buf[i]["obs"] for i in range(self.N)])

        def cat(key):
            return torch.cat(
                [buf[i][key].detach() for i in range(self.N)]
            ).to(self.device, self.dtype).contiguous()

        self.acts = cat("acts")
        self.old_logp = cat("logp")
        self.rtgs = cat("rtgs")
        self.adv = cat("adv")
        # the critic's target: the lambda-returns where the problem
        # carries them (critic_target "lambda"), else the rewards-to-go
        self.vtarg = cat("vtarg") if "vtarg" in buf[0] else self.rtgs

    def load_device_rollout(self, ro):
        """Adopt the ``[N*M, .]`` tensors of ``DeviceRollout.run`` as
        they are (no copies; ``ro["adv"]``, and ``ro["vtarg"]`` under
        ``critic_target: "lambda"``, once the problem has filled them in
        - :meth:`values` needs the observations only)."""
        M = int(ro["M"])
        for key in ("obs", "acts", "logp", "rtgs"):
            t = ro[key]
            assert t.shape[0] == self.N * M and t.is_contiguous()
            assert t.dtype == self.dtype and t.is_cuda
        self.obs = ro["obs"]
        self.acts = ro["acts"]
        self.old_logp = ro["logp"]
        self.rtgs = ro["rtgs"]
        self.vtarg = ro.get("vtarg", self.rtgs)
        assert self.vtarg.shape == self.rtgs.shape
        assert self.vtarg.is_contiguous() and self.vtarg.dtype == self.dtype
        if "adv" in ro:
            self.adv = ro["adv"].contiguous()
        if M != self.M:
            self._alloc(M)

    def load_obs(self, obs_list):
        """Stack per-node observations only (enough for :meth:`values`)."""
        M = int(obs_list[0].shape[0])
        assert all(int(o.shape[0]) == M for o in obs_list)
        self.obs = torch.cat(
            [o.detach() for o in obs_list]
        ).to(self.device, self.dtype).contiguous()
        if M != self.M:
            self._alloc(M)

    # ------------------------------------------------------------------
    def _forward(self, plan, bufs, theta, x=None, rows=None):
        """The net of ``plan`` on ``x`` (``rows`` rows per node), by
        default on the loaded rollout's observations."""
        cur = self.obs if x is None else x
        rows = self.M if rows is None else rows
        for li, layer in enumerate(plan):
            out = bufs["acts"][li]
            self.ext.linear_fwd(
                cur, theta, out, None, layer.w_off, layer.b_off, rows,
                layer.in_dim, layer.out_dim, ACT_IDS[layer.activation],
                layer.scale,
            )
            cur = out
        return cur

    def _backward(self, plan, bufs, theta):
        """dW/db of every layer into ``self.grad``; ``dzs[-1]`` holds the
        loss gradient w.r.t. the net's output on entry. The below
        layer's activation backward rides the dX epilogue, as in
        ``StackedEngine.backward``."""
        ext = self.ext
        for li in range(len(plan) - 1, -1, -1):
            layer = plan[li]
            below = bufs["acts"][li - 1] if li > 0 else self.obs
            dz = bufs["dzs"][li]
            ext.linear_bwd_dw(
                dz, below, self.grad, layer.w_off, layer.b_off, self.M,
                layer.in_dim, layer.out_dim,
            )
            if li > 0:
                lb = plan[li - 1]
                ext.linear_bwd_dx(
                    dz, theta, bufs["dzs"][li - 1], bufs["acts"][li - 1],
                    None, ACT_IDS[lb.activation], lb.scale, layer.w_off,
                    self.M, layer.in_dim, layer.out_dim, None, 0, 0, 0,
                )

    def _check_theta(self, theta):
        theta = self.theta if theta is None else theta
        assert theta.shape == (self.N, self.n) and theta.is_contiguous()
        assert theta.dtype == self.dtype
        return theta

    # ------------------------------------------------------------------
    def grads(self, theta=None, loss_scale=1.0):
        """``[N, n]`` gradient stack of every node's PPO objective at
        ``theta`` on the loaded rollout (returns ``self.grad``)."""
        theta = self._check_theta(theta)
        conf = self.pr.conf
        mean = self._forward(self.actor_plan, self._actor_bufs, theta)
        v = self._forward(self.critic_plan, self._critic_bufs, theta)
        self._loss.zero_()
        self.ext.ppo_loss_bwd(
            mean, self.acts, self.old_logp, self.adv, v.reshape(-1),
            self.vtarg, self._actor_bufs["dzs"][-1],
            self._critic_bufs["dzs"][-1].reshape(-1), self._loss, self.M,
            float(conf["cov"]), float(conf["clip"]),
            float(conf["critic_coef"]), float(loss_scale),
        )
        if self._zero_grad:
            self.grad.zero_()
        self._backward(self.actor_plan, self._actor_bufs, theta)
        self._backward(self.critic_plan, self._critic_bufs, theta)
        return self.grad

    def values(self, theta=None):
        """Critic forward only: ``V(obs)`` as ``[N, M]``."""
        theta = self._check_theta(theta)
        v = self._forward(self.critic_plan, self._critic_bufs, theta)
        return v.reshape(self.N, self.M).clone()

    def values_last(self, theta, last_obs):
        """Critic forward on the observations after the episodes' ends,
        ``last_obs [N*E, obs_dim]`` (row ``l*E + e``, the layout of
        ``DeviceRollout.run``): ``V_end`` as ``[N, E]``. The activations
        go to small buffers of their own, so the loaded rollout, its
        ``M``-row buffers and ``self.obs`` stay as they are.

        ``linear_fwd`` picks its kernel from the row count: the MFMA and
        the small-``I`` kernels want ``M >= 128`` / ``M >= 1024`` rows
        and are never chosen for fewer; ``E`` rows per node down to 1
        take the generic 16x16-tile kernel, which bounds-checks every
        row, as does the MFMA kernel for an ``E`` of 128 and more."""
        theta = self._check_theta(theta)
        N = self.N
        assert last_obs.dim() == 2 and last_obs.shape[0] % N == 0
        E = last_obs.shape[0] // N
        assert E >= 1 and last_obs.shape[1] == self.critic_plan[0].in_dim
        x = last_obs.detach().to(self.device, self.dtype).contiguous()
        if E not in self._last_bufs:
            self._last_bufs[E] = {
                "acts": [
                    torch.empty(N * E, layer.out_dim, device=self.device,
                                dtype=self.dtype)
                    for layer in self.critic_plan
                ]
            }
        v = self._forward(
            self.critic_plan, self._last_bufs[E], theta, x=x, rows=E
        )
        return v.reshape(N, E).clone()

    def losses(self):
        """``[N, 2]`` (actor term, critic term) of the last
        :meth:`grads` call."""
        return self._loss
