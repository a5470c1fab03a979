"""GPU tests of the batched PPO gradient path: ``ext.ppo_loss_bwd``
against autograd, ``StackedPPOEngine`` against the per-node
``local_batch_loss(i).backward()``, and one round of each PPO optimizer
with ``grad_engine="stacked"`` against ``"torch"``."""

import copy
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

pytestmark = pytest.mark.gpu

requires_gpu = pytest.mark.skipif(
    not torch.cuda.is_available(), reason="needs MI355X"
)

# the table of tests/test_ops_gpu.py
TOL = {torch.float64: dict(rtol=1e-10, atol=1e-10),
       torch.float32: dict(rtol=2e-4, atol=2e-5)}
# one DiNNO/DSGD/DSGT round, as test_dinno_ppo_hip_round_matches_torch
ROUND_TOL = dict(rtol=2e-4, atol=2e-5)

COV, CLIP, CRITIC_COEF = 0.5, 0.2, 0.5
R_TARGETS = (0.5, 0.9, 1.1, 1.5)


@pytest.fixture(scope="module")
def ext():
    from nn_distributed_training_amd.ops import get_ext

    return get_ext()


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


def _dev():
    return torch.device("cuda")


def _targets(rows, gen):
    """Per-row (log target ratio, advantage sign): the four targets x
    both signs dealt round-robin, so every region is hit from 8 rows
    on, then shuffled."""
    k = torch.arange(rows)
    perm = torch.randperm(rows, generator=gen)
    log_r = torch.tensor([math.log(r) for r in R_TARGETS])[k % 4][perm]
    sign = (1.0 - 2.0 * ((k // 4) % 2))[perm]
    return log_r, sign


def _assert_regions(ratios, adv):
    """Every sample is clear of the clip bounds by 1e-3 (fp32 rounding
    cannot move it across) and all six regions are populated."""
    lo, hi = 1 - CLIP, 1 + CLIP
    assert ((ratios - lo).abs() >= 1e-3).all()
    assert ((ratios - hi).abs() >= 1e-3).all()
    for sel in (adv > 0, adv < 0):
        assert (sel & (ratios < lo)).any()
        assert (sel & (ratios > hi)).any()
        assert (sel & (ratios > lo) & (ratios < hi)).any()


@requires_gpu
@both_dtypes
@pytest.mark.parametrize("L,M,A", [(3, 37, 5), (2, 300, 5)])
def test_ppo_loss_bwd_matches_autograd(ext, dtype, L, M, A):
    """(3, 37, 5): rows no multiple of wave or block, node boundaries
    inside a wave. (2, 300, 5): a block boundary inside a node, and
    waves that reduce by shuffle."""
    dev = _dev()
    gen = torch.Generator().manual_seed(11)
    rows = L * M
    loss_scale = 0.7
    mean = torch.randn(rows, A, generator=gen).to(dev)
    acts = (mean.cpu() + math.sqrt(COV) * torch.randn(
        rows, A, generator=gen)).to(dev)
    log_r, sign = _targets(rows, gen)
    adv = (sign * (0.2 + torch.rand(rows, generator=gen))).to(dev)
    v = torch.randn(rows, generator=gen).to(dev)
    rtgs = torch.randn(rows, generator=gen).to(dev)
    cov_mat = torch.eye(A, device=dev) * COV

    mean_r = mean.clone().requires_grad_(True)
    v_r = v.clone().requires_grad_(True)
    logp = MultivariateNormal(mean_r, cov_mat).log_prob(acts)
    old_logp = (logp.detach() - log_r.to(dev)).contiguous()
    ratios = torch.exp(logp - old_logp)
    _assert_regions(ratios.detach(), adv)
    s1 = ratios * adv
    s2 = torch.clamp(ratios, 1 - CLIP, 1 + CLIP) * adv
    actor = -torch.min(s1, s2).reshape(L, M).mean(dim=1)
    critic = ((v_r - rtgs) ** 2).reshape(L, M).mean(dim=1)
    (loss_scale * (actor + CRITIC_COEF * critic).sum()).backward()
    ref_loss = torch.stack([actor, critic], dim=1).detach()

    dmean = torch.full_like(mean, float("nan"))
    dv = torch.full_like(v, float("nan"))
    loss = torch.zeros(L, 2, device=dev)
    ext.ppo_loss_bwd(mean, acts, old_logp, adv, v, rtgs, dmean, dv,
                     loss, M, COV, CLIP, CRITIC_COEF, loss_scale)
    print(f"max |dmean - ref| = {(dmean - mean_r.grad).abs().max():.3e}"
          f", |dv - ref| = {(dv - v_r.grad).abs().max():.3e}"
          f", |loss - ref| = {(loss - ref_loss).abs().max():.3e}")
    torch.testing.assert_close(dmean, mean_r.grad, **TOL[dtype])
    torch.testing.assert_close(dv, v_r.grad, **TOL[dtype])
    torch.testing.assert_close(loss, ref_loss, **TOL[dtype])

    # without a loss buffer the gradients are the same numbers
    dmean2 = torch.full_like(mean, float("nan"))
    dv2 = torch.full_like(v, float("nan"))
    ext.ppo_loss_bwd(mean, acts, old_logp, adv, v, rtgs, dmean2, dv2,
                     None, M, COV, CLIP, CRITIC_COEF, loss_scale)
    assert torch.equal(dmean2, dmean) and torch.equal(dv2, dv)


@requires_gpu
def test_ppo_loss_bwd_rejects_wide_actions(ext):
    dev = _dev()
    z = torch.zeros(4, 17, device=dev)
    s = torch.zeros(4, device=dev)
    with pytest.raises(RuntimeError, match="action dim"):
        ext.ppo_loss_bwd(z, z, s, s, s, s, z.clone(), s.clone(), None,
                         4, COV, CLIP, CRITIC_COEF, 1.0)


# ----------------------------------------------------------------------
def _problem(hidden, M, seed=0):
    """DistPPOProblem on wheel_graph(3) whose rollout buffers are seeded
    random tensors (no rollout): old_logp puts the ratios on the four
    targets, so both clip regions occur for both advantage signs."""
    torch.manual_seed(seed)
    dev = _dev()
    env = SimpleTagEnv(num_predators=3, num_obstacles=1, seed=0,
                       max_steps=20)
    conf = {"hidden": hidden, "verbose": False, "cov": COV,
            "clip": CLIP, "critic_coef": CRITIC_COEF}
    pr = DistPPOProblem(nx.wheel_graph(3), env, dev, conf)
    # distinct parameters per node (the constructor deep-copies one net)
    for i in range(pr.N):
        with torch.no_grad():
            for p in pr.node_parameters(i):
                p.add_(0.1 * torch.randn_like(p))
    gen = torch.Generator().manual_seed(seed + 1)
    pr.buf = {}
    for i in range(pr.N):
        obs = torch.randn(M, env.obs_dim, generator=gen).to(dev)
        with torch.no_grad():
            mean = pr.actors[i](obs)
            acts = mean + math.sqrt(COV) * torch.randn(
                M, env.act_dim, generator=gen).to(dev)
            logp = MultivariateNormal(mean, pr.cov_mat).log_prob(acts)
        log_r, sign = _targets(M, gen)
        adv = (sign * (0.2 + torch.rand(M, generator=gen))).to(dev)
        _assert_regions(torch.exp(log_r), sign)
        pr.buf[i] = dict(
            obs=obs, acts=acts, logp=logp - log_r.to(dev),
            rtgs=torch.randn(M, generator=gen).to(dev), adv=adv,
        )
    return pr


def _autograd_grads(pr):
    rows = []
    for i in range(pr.N):
        for p in pr.node_parameters(i):
            p.grad = None
        pr.local_batch_loss(i).backward()
        rows.append(
            torch.cat([p.grad.reshape(-1) for p in pr.node_parameters(i)])
        )
    return torch.stack(rows)


# hidden=(16, 16), M=60: the small-tile VALU kernels only.
# hidden=(64, 64, 64), M=260: M no multiple of 64, partial MFMA tiles,
# I=12 first layers, O=5 / O=1 last layers, accumulating dW kernels.
ENGINE_SHAPES = [((16, 16), 60), ((64, 64, 64), 260)]


@requires_gpu
@both_dtypes
@pytest.mark.parametrize("hidden,M", ENGINE_SHAPES)
def test_engine_grads_match_per_node_autograd(dtype, hidden, M):
    from nn_distributed_training_amd.rl.stacked_ppo import (
        StackedPPOEngine,
    )

    pr = _problem(hidden, M)
    ref = _autograd_grads(pr)
    eng = StackedPPOEngine(pr)
    assert eng.theta.shape == (3, pr.n)
    eng.load_rollout(pr.buf)
    g1 = eng.grads().clone()
    loss1 = eng.losses().clone()
    # a second call must not add onto the first (accumulating dW paths)
    g2 = eng.grads().clone()
    print(f"max |grad - ref| = {(g1 - ref).abs().max():.3e} "
          f"(second call {(g2 - ref).abs().max():.3e}), "
          f"max |ref| = {ref.abs().max():.3e}")
    for i in range(pr.N):
        torch.testing.assert_close(g1[i], ref[i], **TOL[dtype])
        torch.testing.assert_close(g2[i], ref[i], **TOL[dtype])
    with torch.no_grad():
        tot = torch.stack([pr.local_batch_loss(i) for i in range(pr.N)])
    torch.testing.assert_close(
        loss1[:, 0] + CRITIC_COEF * loss1[:, 1], tot, **TOL[dtype]
    )
    # grads at an explicitly passed stack: the parameters of the
    # modules rolled by one node
    theta = eng.theta.roll(1, dims=0).contiguous()
    g3 = eng.grads(theta).clone()
    for i in range(pr.N):
        pr.set_node_vector(i, theta[i].clone())
    ref3 = _autograd_grads(pr)
    for i in range(pr.N):
        torch.testing.assert_close(g3[i], ref3[i], **TOL[dtype])


@requires_gpu
@both_dtypes
@pytest.mark.parametrize("hidden,M", ENGINE_SHAPES)
def test_engine_values_match_critics(dtype, hidden, M):
    from nn_distributed_training_amd.rl.stacked_ppo import (
        StackedPPOEngine,
    )

    pr = _problem(hidden, M, seed=2)
    eng = StackedPPOEngine(pr)
    eng.load_rollout(pr.buf)
    v = eng.values()
    assert v.shape == (3, M)
    for i in range(pr.N):
        with torch.no_grad():
            ref = pr.critics[i](pr.buf[i]["obs"]).squeeze(-1)
        torch.testing.assert_close(v[i], ref, **TOL[dtype])


# ----------------------------------------------------------------------
ROUND_CONF = {
    "timesteps_per_batch": 60,
    "max_timesteps_per_episode": 20,
    "hidden": (16, 16),
    "verbose": False,
    # dinno
    "rho_init": 0.2, "primal_iterations": 3, "expected_iterations": 10,
    "primal_lr_start": 1e-3, "primal_lr_finish": 1e-4,
    # dsgd / dsgt
    "alpha0": 1e-2, "mu": 1e-3, "alpha_actor": 1e-2,
    "alpha_critic": 5e-3,
}


@pytest.fixture
def fp32():
    # RL runs in fp32, as in tests/test_rl.py
    prev = torch.get_default_dtype()
    torch.set_default_dtype(torch.float32)
    yield
    torch.set_default_dtype(prev)


def _rolled_out_problem():
    torch.manual_seed(0)
    env = SimpleTagEnv(num_predators=3, num_obstacles=1, seed=0,
                       max_steps=20)
    pr = DistPPOProblem(nx.wheel_graph(3), env, _dev(), ROUND_CONF)
    for i in range(pr.N):
        with torch.no_grad():
            for p in pr.node_parameters(i):
                p.add_(0.05 * torch.randn_like(p))
    pr.rollout()
    return pr


@requires_gpu
@pytest.mark.parametrize("alg", ["dinno", "dsgd", "dsgt"])
def test_round_stacked_matches_torch(fp32, alg):
    pr1 = _rolled_out_problem()
    pr2 = copy.deepcopy(pr1)
    before = [pr1.node_vector(i).detach().clone() for i in range(3)]

    o1 = build_ppo_optimizer(alg, pr1, {**ROUND_CONF,
                                        "grad_engine": "torch"})
    o2 = build_ppo_optimizer(alg, pr2, {**ROUND_CONF,
                                        "grad_engine": "stacked"})
    assert o1.grad_engine == "torch" and o1.engine is None
    assert o2.grad_engine == "stacked" and o2.engine is not None
    o1.step_round(0)
    o2.step_round(0)

    for i in range(3):
        # the modules hold the round's result
        got = torch.cat([p.detach().reshape(-1)
                         for p in pr2.node_parameters(i)])
        assert not torch.equal(got, before[i])
        torch.testing.assert_close(
            got, pr1.node_vector(i).detach(), **ROUND_TOL
        )
        if alg == "dinno":
            torch.testing.assert_close(
                o2.duals[i], o1.duals[i], **ROUND_TOL
            )
        if alg == "dsgt":
            torch.testing.assert_close(o2.y[i], o1.y[i], **ROUND_TOL)
            torch.testing.assert_close(o2.g[i], o1.g[i], **ROUND_TOL)


@requires_gpu
def test_rollout_advantages_from_engine_values(fp32):
    """With the stacked engine attached, rollout() normalizes
    rtg - V(obs) batched over [N, M] with V from engine.values; the
    buffers equal the per-node computation."""
    pr = _rolled_out_problem()
    opt = build_ppo_optimizer("dsgd", pr, {**ROUND_CONF,
                                           "grad_engine": "stacked"})
    assert pr.value_engine is opt.engine
    pr.rollout()
    for i in range(pr.N):
        b = pr.buf[i]
        with torch.no_grad():
            adv = b["rtgs"] - pr.critics[i](b["obs"]).squeeze(-1)
        adv = (adv - adv.mean()) / (adv.std() + 1e-10)
        torch.testing.assert_close(b["adv"], adv, **TOL[torch.float32])
