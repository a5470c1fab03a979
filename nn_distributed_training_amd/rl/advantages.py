"""GAE(lambda) advantages for the multi-agent PPO tree.

For node ``l`` and an episode covering steps ``s .. s + len - 1`` of the
node's batch of ``M`` steps (an episode's end is terminal: no bootstrap,
the convention of ``DistPPOProblem``'s rewards-to-go)::

    delta_s = r_s + gamma * V_{s+1} * [s+1 in the episode] - V_s
    A_s     = delta_s + gamma*lam * A_{s+1} * [s+1 in the episode]
    ret_s   = A_s + V_s                       (the lambda-return)
    adv_s   = (A_s - mean_l A) / (std_l A + 1e-10)

With ``lam = 1`` the sum telescopes to ``A_s = rtg_s - V_s`` and ``ret_s =
rtg_s``: the Monte-Carlo estimator ``DistPPOProblem`` uses by default.

:func:`gae_advantages_torch` is the recurrence in plain torch, for any
list of episode lengths: the documentation of what ``ppo_gae_k``
(ops/hip/advantage.hip) computes, the oracle of the tests, and the
implementation wherever the kernel is not used. :func:`gae_advantages_hip`
launches the kernel, which takes uniform episodes (the layout of
rl/device_rollout.py) and normalises in the same launch.
"""

from __future__ import annotations

import torch

# the kernel's limit, the rollout kernel's as well (rl/device_rollout.py)
MAX_EP_LEN = 4096


def uniform_ep_len(ep_lens):
    """``ep_len`` when ``ep_lens`` is the device rollout's layout (every
    episode ``ep_len`` steps long, the last one at most that), else
    None."""
    ep_lens = [int(n) for n in ep_lens]
    ep_len = ep_lens[0]
    if any(n != ep_len for n in ep_lens[:-1]):
        return None
    if not 1 <= ep_lens[-1] <= ep_len:
        return None
    return ep_len


def gae_advantages_torch(v, rews, ep_lens, gamma, lam):
    """``(A, ret)``, both ``[L, M]`` double and NOT normalised, from the
    critic values ``v [L, M]``, the rewards ``rews`` (``[L, M]``, or
    ``[M]`` for a reward shared by all nodes) and the episode lengths
    ``ep_lens`` (they sum to ``M``; ragged lengths are fine). The
    arithmetic is double whatever ``v``'s dtype, as in the kernel."""
    L, M = v.shape
    ep_lens = [int(n) for n in ep_lens]
    if min(ep_lens) < 1 or sum(ep_lens) != M:
        raise ValueError(
            f"episode lengths {ep_lens} do not partition {M} steps"
        )
    v = v.detach().to(torch.float64)
    rews = rews.detach().to(v.device, torch.float64).expand(L, M)
    # cont[s]: step s+1 belongs to the episode of step s
    cont = [1.0] * M
    s = 0
    for n in ep_lens:
        s += n
        cont[s - 1] = 0.0
    cont_t = torch.tensor(cont, dtype=torch.float64, device=v.device)
    v_next = torch.cat([v[:, 1:], torch.zeros_like(v[:, :1])], dim=1)
    delta = rews + gamma * v_next * cont_t - v
    A = torch.empty_like(v)
    run = torch.zeros(L, dtype=torch.float64, device=v.device)
    c = gamma * lam
    for s in range(M - 1, -1, -1):
        run = delta[:, s] + (c * cont[s]) * run
        A[:, s] = run
    return A, A + v


def normalize_advantages(A):
    """Per-row normalisation: zero mean, unit (unbiased) std over each
    node's ``M`` rows."""
    return (A - A.mean(dim=-1, keepdim=True)) / (
        A.std(dim=-1, keepdim=True) + 1e-10
    )


def gae_advantages_hip(v, rews, ep_len, gamma, lam, want_ret=True):
    """One ``ext.ppo_gae`` launch: ``(adv, ret)`` as ``[L, M]`` of
    ``v``'s dtype, ``adv`` already normalised per node, ``ret`` None
    unless ``want_ret``. ``v`` is ``[L, M]`` on the GPU, ``rews`` double,
    ``[M]`` (shared by all nodes) or ``[L, M]``; episodes of ``ep_len``
    steps, the last one cut at ``M``. Arguments the kernel does not take
    are a ``ValueError``."""
    from ..ops import get_ext

    if v.dim() != 2:
        raise ValueError("v must be [L, M]")
    L, M = v.shape
    ep_len = int(ep_len)
    if M < 2:
        raise ValueError(f"GAE kernel needs at least 2 steps, got {M}")
    if not 1 <= ep_len <= MAX_EP_LEN:
        raise ValueError(
            f"GAE kernel supports episodes of 1..{MAX_EP_LEN} steps, "
            f"got {ep_len}"
        )
    if not (0.0 <= gamma <= 1.0 and 0.0 <= lam <= 1.0):
        raise ValueError(
            f"gamma and lambda must be in [0, 1], got {gamma}, {lam}"
        )
    if v.dtype not in (torch.float32, torch.float64):
        raise ValueError(f"GAE kernel supports fp32/fp64, got {v.dtype}")
    if rews.dtype != torch.float64:
        raise ValueError(f"rews must be double, got {rews.dtype}")
    if not (v.is_cuda and rews.is_cuda):
        raise ValueError("GAE kernel needs its tensors on the GPU")
    if tuple(rews.shape) == (M,):
        stride = 0
    elif tuple(rews.shape) == (L, M):
        stride = M
    else:
        raise ValueError(
            f"rews must be [{M}] or [{L}, {M}], got {tuple(rews.shape)}"
        )
    v = v.detach().contiguous()
    adv = torch.empty_like(v)
    ret = torch.empty_like(v) if want_ret else None
    get_ext().ppo_gae(
        v.view(-1), rews.detach().contiguous().view(-1), stride,
        adv.view(-1), None if ret is None else ret.view(-1), M, ep_len,
        float(gamma), float(lam),
    )
    return adv, ret
