"""GPU tests of the one-launch PPO gradient kernel (``ppo_grad_fused_k``,
``grad_engine: "fused"``): ``FusedPPOEngine.grads`` against fp64
autograd, one round of each PPO optimizer against ``"torch"``, and the
refusal of nets outside the kernel's limits."""

import copy

import pytest
import torch

from nn_distributed_training_amd.rl.ppo_optimizers import (
    build_ppo_optimizer,
)
from test_ppo_stacked_gpu import (  # noqa: F401  (dtype, fp32: fixtures)
    CRITIC_COEF, ROUND_CONF, ROUND_TOL, TOL, _autograd_grads, _problem,
    _rolled_out_problem, both_dtypes, dtype, fp32, requires_gpu,
)

pytestmark = pytest.mark.gpu


def _fp64_copy(pr):
    """The problem in double: the reference of either dtype's run."""
    ref = copy.deepcopy(pr)
    for net in list(ref.actors.values()) + list(ref.critics.values()):
        net.double()
    ref.cov_mat = ref.cov_mat.double()
    ref.buf = {i: {k: v.double() for k, v in b.items()}
               for i, b in ref.buf.items()}
    return ref


# (16, 16), 37: one fragment per layer, one partial tile at 64 rows and
#   ragged tiles at 16; in = 12 and the heads 5 / 1 padded to 16.
# (48, 24), 70: unequal widths, 24 no multiple of 16 (K and O padding in
#   one layer), two tiles at 64 rows.
# (64, 64, 64), 130: the widest net, three tiles at 64 rows, the last
#   with 2 rows: the slab reduce and the ticket.
FUSED_SHAPES = [((16, 16), 37), ((48, 24), 70), ((64, 64, 64), 130)]


@requires_gpu
@both_dtypes
@pytest.mark.parametrize("hidden,M", FUSED_SHAPES)
def test_fused_grads_match_fp64_autograd(dtype, hidden, M):
    from nn_distributed_training_amd.rl.stacked_ppo import FusedPPOEngine

    pr = _problem(hidden, M)
    ref_pr = _fp64_copy(pr)
    ref = _autograd_grads(ref_pr)
    with torch.no_grad():
        ref_loss = torch.stack(
            [ref_pr.local_batch_loss(i) for i in range(pr.N)])
    eng = FusedPPOEngine(pr)
    eng.load_rollout(pr.buf)
    g1 = eng.grads().clone()
    loss1 = eng.losses().clone()
    print(f"max |grad - ref| = {(g1 - ref).abs().max():.3e}, "
          f"max |ref| = {ref.abs().max():.3e}")
    for i in range(pr.N):
        torch.testing.assert_close(g1[i], ref[i].to(dtype), **TOL[dtype])
    torch.testing.assert_close(
        loss1[:, 0] + CRITIC_COEF * loss1[:, 1], ref_loss.to(dtype),
        **TOL[dtype])
    # overwrite, ticket reset and determinism: nothing of the buffers'
    # earlier content survives and the bits repeat
    eng.grad.fill_(float("nan"))
    eng.losses().fill_(float("nan"))
    assert torch.equal(eng.grads(), g1)
    assert torch.equal(eng.losses(), loss1)
    # grads at an explicitly passed stack: the modules' parameters
    # rolled by one node
    theta = eng.theta.roll(1, dims=0).contiguous()
    g3 = eng.grads(theta).clone()
    for i in range(pr.N):
        ref_pr.set_node_vector(i, theta[i].double())
    ref3 = _autograd_grads(ref_pr)
    print(f"rolled: max |grad - ref| = {(g3 - ref3).abs().max():.3e}")
    for i in range(pr.N):
        torch.testing.assert_close(g3[i], ref3[i].to(dtype), **TOL[dtype])


@requires_gpu
@pytest.mark.parametrize("alg", ["dinno", "dsgd", "dsgt"])
def test_round_fused_matches_torch(fp32, alg):
    pr1 = _rolled_out_problem()
    pr2 = copy.deepcopy(pr1)
    before = [pr1.node_vector(i).detach().clone() for i in range(3)]
    o1 = build_ppo_optimizer(alg, pr1, {**ROUND_CONF,
                                        "grad_engine": "torch"})
    o2 = build_ppo_optimizer(alg, pr2, {**ROUND_CONF,
                                        "grad_engine": "fused"})
    assert type(o2.engine).__name__ == "FusedPPOEngine"
    o1.step_round(0)
    o2.step_round(0)
    for i in range(3):
        got = pr2.node_vector(i).detach()
        assert not torch.equal(got, before[i])
        torch.testing.assert_close(
            got, pr1.node_vector(i).detach(), **ROUND_TOL)
        if alg == "dinno":
            torch.testing.assert_close(
                o2.duals[i], o1.duals[i], **ROUND_TOL)
        if alg == "dsgt":
            torch.testing.assert_close(o2.y[i], o1.y[i], **ROUND_TOL)
            torch.testing.assert_close(o2.g[i], o1.g[i], **ROUND_TOL)


@requires_gpu
def test_fused_refuses_wide_nets(fp32):
    pr = _problem((128,), 20)
    with pytest.raises(ValueError, match="width"):
        build_ppo_optimizer("dsgd", pr, {**ROUND_CONF,
                                         "grad_engine": "fused"})
    assert pr.value_engine is None
