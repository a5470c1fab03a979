"""CPU tests of the batched PPO gradient path: the pure-torch mirror of
``ppo_loss_bwd_k`` against autograd of ``local_batch_loss``'s own
expressions, and the ``grad_engine`` switch of the PPO optimizers."""

import math

import networkx as nx
import pytest
import torch
from torch.distributions import MultivariateNormal

from nn_distributed_training_amd.rl.dist_ppo import DistPPOProblem
from nn_distributed_training_amd.rl.envs import SimpleTagEnv
from nn_distributed_training_amd.rl.ppo_optimizers import (
    build_ppo_optimizer,
)
from nn_distributed_training_amd.rl.stacked_ppo import (
    ppo_loss_grads_torch,
)

L, M, A = 2, 11, 5
COV, CRITIC_COEF, LOSS_SCALE = 0.5, 0.5, 0.7
# candidates for |log ratio| of the samples placed exactly on a clip
# bound: multiples of 2^-7, which logp -/+ x reproduces without rounding
X_TIES = (0.25, 0.1875, 0.21875, 0.203125, 0.234375, 0.2421875)


def _tie_log_ratio(sign):
    """A log-ratio x whose exp() has one value however torch evaluates
    it (vector lanes and the scalar remainder loop may round exp
    differently; the reference slices per node, the mirror does not)."""
    for q in X_TIES:
        x = sign * q
        outs = {math.exp(x)}
        for n in (1, M, L * M):
            outs |= set(
                torch.exp(torch.full((n,), x, dtype=torch.float64))
                .tolist()
            )
        if len(outs) == 1:
            return x
    raise AssertionError("no candidate log-ratio with a unique exp()")
# (target ratio, advantage sign) per row of one node: the six
# (ratio region x advantage sign) cases, the two ties on the bound under
# test, and three more inside/outside samples
REGIONS = [(0.5, 1), (0.5, -1), (0.9, 1), (1.1, -1), (1.5, 1), (1.5, -1)]
EXTRA = [(1.05, 1), (0.6, -1), (1.7, 1)]


def _autograd_reference(mean, acts, old_logp, adv, v, rtgs, clip):
    """The expressions of DistPPOProblem.local_batch_loss, per node,
    with the two nets' outputs as leaves."""
    mean = mean.clone().requires_grad_(True)
    v = v.clone().requires_grad_(True)
    cov_mat = torch.eye(A, dtype=mean.dtype) * COV
    total = 0.0
    losses = []
    for l in range(L):
        s = slice(l * M, (l + 1) * M)
        dist = MultivariateNormal(mean[s], cov_mat)
        logp = dist.log_prob(acts[s])
        ratios = torch.exp(logp - old_logp[s])
        s1 = ratios * adv[s]
        s2 = torch.clamp(ratios, 1 - clip, 1 + clip) * adv[s]
        actor_loss = -torch.min(s1, s2).mean()
        critic_loss = torch.nn.functional.mse_loss(v[s], rtgs[s])
        total = total + actor_loss + CRITIC_COEF * critic_loss
        losses.append(torch.stack([actor_loss, critic_loss]))
    (LOSS_SCALE * total).backward()
    return mean.grad, v.grad, torch.stack(losses).detach()


@pytest.mark.parametrize("bound", ["lower", "upper"])
def test_formula_mirror_matches_autograd(bound):
    """ppo_loss_grads_torch against autograd in fp64, with samples in
    all six regions and, for both advantage signs, samples whose ratio
    sits EXACTLY on the clip bound under test: there torch's minimum
    splits the tie and clamp still passes the gradient, which is where
    a hand-written subgradient usually differs.

    An exact tie needs exp(logp - old_logp) == 1 -/+ clip to the last
    bit in both computations, so the tie rows are drawn from candidates
    whose closed-form logp equals MultivariateNormal's bitwise, their
    log-ratio is an exactly representable -/+x, and clip is set from
    the ratio torch computes for them (1 - (1 - r) and 1 + (r - 1) are
    exact for r in [0.5, 2]). One bound per case, since one clip cannot
    put exp(-x) and exp(+x) on both bounds at once."""
    g = torch.Generator().manual_seed(3)
    dt = torch.float64
    K = 512
    mean_c = torch.randn(K, A, generator=g, dtype=dt)
    acts_c = mean_c + math.sqrt(COV) * torch.randn(
        K, A, generator=g, dtype=dt
    )
    lp_mvn = MultivariateNormal(
        mean_c, torch.eye(A, dtype=dt) * COV
    ).log_prob(acts_c)
    d = acts_c - mean_c
    lp_formula = (
        -0.5 * (d * d).sum(dim=1) / COV
        - 0.5 * A * math.log(2 * math.pi * COV)
    )
    x_tie = _tie_log_ratio(-1 if bound == "lower" else 1)
    exact = (lp_mvn == lp_formula) & (
        lp_mvn - (lp_mvn - x_tie) == x_tie
    )
    same = torch.nonzero(exact).reshape(-1)
    other = torch.nonzero(~exact).reshape(-1)
    assert same.numel() >= 2 * L and other.numel() >= (M - 2) * L

    rows, log_r, sign, tie = [], [], [], []
    for l in range(L):
        for k, (rt, sg) in enumerate(REGIONS + EXTRA):
            rows.append(int(other[l * (M - 2) + k]))
            log_r.append(math.log(rt))
            sign.append(sg)
            tie.append(False)
        for k, sg in enumerate((1, -1)):
            rows.append(int(same[2 * l + k]))
            log_r.append(x_tie)
            sign.append(sg)
            tie.append(True)
    rows = torch.tensor(rows)
    tie = torch.tensor(tie)
    mean, acts = mean_c[rows], acts_c[rows]
    old_logp = lp_mvn[rows] - torch.tensor(log_r, dtype=dt)
    adv = torch.tensor(sign, dtype=dt) * (
        0.2 + torch.rand(L * M, generator=g, dtype=dt)
    )
    v = torch.randn(L * M, generator=g, dtype=dt)
    rtgs = torch.randn(L * M, generator=g, dtype=dt)

    ratios = torch.exp(lp_mvn[rows] - old_logp)
    r_tie = ratios[tie]
    assert (r_tie == r_tie[0]).all()
    clip = float(1 - r_tie[0]) if bound == "lower" else float(r_tie[0] - 1)
    lo, hi = 1 - clip, 1 + clip
    edge = lo if bound == "lower" else hi
    # the ties are exact in BOTH computations of the ratio
    assert (ratios[tie] == edge).all()
    assert (torch.exp(lp_formula[rows] - old_logp)[tie] == edge).all()
    assert 0.15 < clip < 0.3
    # and the six regions are all present
    for sg in (1, -1):
        sel = torch.tensor(sign) == sg
        assert (sel & (ratios < lo)).any()
        assert (sel & (ratios > hi)).any()
        assert (sel & (ratios > lo) & (ratios < hi)).any()

    ref_dmean, ref_dv, ref_loss = _autograd_reference(
        mean, acts, old_logp, adv, v, rtgs, clip
    )
    dmean, dv, loss = ppo_loss_grads_torch(
        mean, acts, old_logp, adv, v, rtgs, M, COV, clip, CRITIC_COEF,
        LOSS_SCALE,
    )
    tol = dict(rtol=1e-10, atol=1e-12)
    torch.testing.assert_close(dmean, ref_dmean, **tol)
    torch.testing.assert_close(dv, ref_dv, **tol)
    torch.testing.assert_close(loss, ref_loss, **tol)
    # the tie rows carry the full advantage (not half, not zero)
    assert (dmean[tie].abs().sum(dim=1) > 0).all()


def _cpu_problem():
    env = SimpleTagEnv(num_predators=3, num_obstacles=1, seed=0,
                       max_steps=20)
    conf = {
        "timesteps_per_batch": 40, "max_timesteps_per_episode": 20,
        "hidden": (8,), "verbose": False,
    }
    pr = DistPPOProblem(
        nx.wheel_graph(3), env, torch.device("cpu"), conf
    )
    return pr, conf


@pytest.mark.parametrize("alg", ["dinno", "dsgd", "dsgt"])
def test_stacked_on_cpu_fails_loudly(alg):
    pr, conf = _cpu_problem()
    with pytest.raises(ValueError, match="grad_engine"):
        build_ppo_optimizer(alg, pr, {**conf, "grad_engine": "stacked"})
    # nothing was attached to the problem on the way out
    assert pr.value_engine is None


@pytest.mark.parametrize("alg", ["dinno", "dsgd", "dsgt"])
def test_grad_engine_defaults_to_torch(alg):
    pr, conf = _cpu_problem()
    opt = build_ppo_optimizer(alg, pr, conf)
    assert opt.grad_engine == "torch"
    assert opt.engine is None and pr.value_engine is None


def test_unknown_grad_engine_rejected():
    pr, conf = _cpu_problem()
    with pytest.raises(ValueError, match="grad_engine"):
        build_ppo_optimizer("dsgd", pr, {**conf, "grad_engine": "hip"})
