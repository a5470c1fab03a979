"""GAE(lambda) advantages for the multi-agent PPO tree.

For node ``l`` and episode ``e`` covering steps ``b .. b + len - 1`` of
the node's batch of ``M`` steps::

    delta_s = r_s + gamma * V_{s+1} - V_s          s not the episode's last
    delta_s = r_s + gamma * V_end[l, e] - V_s      s the episode's last
    A_s     = delta_s + gamma*lam * A_{s+1} * [s+1 in the episode]
    ret_s   = A_s + V_s                       (the lambda-return)
    adv_s   = (A_s - mean_l A) / (std_l A + 1e-10)

By default ``V_end = 0``: an episode's end is terminal (no bootstrap), the
convention of ``DistPPOProblem``'s rewards-to-go. With ``lam = 1`` the sum
then telescopes to ``A_s = rtg_s - V_s`` and ``ret_s = rtg_s``: the
Monte-Carlo estimator ``DistPPOProblem`` uses by default.

``SimpleTagEnv``'s episodes end only at a step limit, though: every end
is a truncation, and a zero beyond it biases the targets of a critic
whose input carries no time index (Pardo et al. 2018, "Time Limits in
Reinforcement Learning"). Partial-episode bootstrapping
(``bootstrap_truncated`` of ``DistPPOProblem``) passes ``v_last [L, E]``,
the critic's value ``V_end[l, e]`` of the observation the env returned
after the episode's last step. The rewards-to-go then continue the same
way (:func:`bootstrap_rtgs`)::

    rtg^b_s = rtg_s + gamma^(b + len - s) * V_end[l, e]

and at ``lam = 1``: ``A_s = rtg^b_s - V_s``, ``ret_s = rtg^b_s``.

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


def gae_advantages_torch(v, rews, ep_lens, gamma, lam, v_last=None):
    """``(A, ret)``, both ``[L, M]`` double and NOT normalised, from the
    critic values ``v [L, M]``, the rewards ``rews`` (``[L, M]``, or
    ``[M]`` for a reward shared by all nodes) and the episode lengths
    ``ep_lens`` (they sum to ``M``; ragged lengths are fine). ``v_last
    [L, len(ep_lens)]`` bootstraps the episodes' ends; None leaves them
    terminal. The arithmetic is double whatever ``v``'s dtype, as in the
    kernel."""
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
    if v_last is not None:
        if tuple(v_last.shape) != (L, len(ep_lens)):
            raise ValueError(
                f"v_last must be [{L}, {len(ep_lens)}], got "
                f"{tuple(v_last.shape)}"
            )
        v_last = v_last.detach().to(v.device, torch.float64)
        # the episodes' last steps, where delta has no V_{s+1} term yet
        ends = torch.tensor(ep_lens, device=v.device).cumsum(0) - 1
        delta[:, ends] = rews[:, ends] + gamma * v_last - v[:, ends]
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


_DISC = {}


def _end_discounts(ep_lens, gamma, device):
    """``(disc, ep)``, both ``[M]``: ``disc[s] = gamma^(b_e + len_e - s)``
    (double), what a value after the last step of ``s``'s episode ``e``
    is worth at ``s``, and ``ep[s] = e``. They depend on ``(ep_lens,
    gamma)`` only, so they are built once per layout and device, not once
    per round."""
    key = (tuple(ep_lens), float(gamma), str(device))
    if key not in _DISC:
        if len(_DISC) >= 16:  # ragged host layouts: no unbounded growth
            _DISC.clear()
        disc = torch.tensor(
            [float(gamma) ** (n - t) for n in ep_lens for t in range(n)],
            dtype=torch.float64,
        )
        ep = torch.tensor(
            [e for e, n in enumerate(ep_lens) for _ in range(n)]
        )
        _DISC[key] = (disc.to(device), ep.to(device))
    return _DISC[key]


def bootstrap_rtgs(rtgs, v_last, ep_lens, gamma):
    """The bootstrapped rewards-to-go ``rtg^b [L, M]`` of ``rtgs``'s
    dtype from the plain ones ``rtgs [L, M]`` and ``v_last [L, E]`` for
    episodes of lengths ``ep_lens``, the sum in double."""
    L, M = rtgs.shape
    ep_lens = [int(n) for n in ep_lens]
    if min(ep_lens) < 1 or sum(ep_lens) != M:
        raise ValueError(
            f"episode lengths {ep_lens} do not partition {M} steps"
        )
    if tuple(v_last.shape) != (L, len(ep_lens)):
        raise ValueError(
            f"v_last must be [{L}, {len(ep_lens)}], got "
            f"{tuple(v_last.shape)}"
        )
    disc, ep = _end_discounts(ep_lens, gamma, rtgs.device)
    tail = v_last.detach().to(rtgs.device, torch.float64)[:, ep]
    return (rtgs.detach().to(torch.float64) + disc * tail).to(rtgs.dtype)


def gae_advantages_hip(v, rews, ep_len, gamma, lam, want_ret=True,
                       v_last=None):
    """One ``ext.ppo_gae`` launch: ``(adv, ret)`` as ``[L, M]`` of
    ``v``'s dtype, ``adv`` already normalised per node, ``ret`` None
    unless ``want_ret``. ``v`` is ``[L, M]`` on the GPU, ``rews`` double,
    ``[M]`` (shared by all nodes) or ``[L, M]``; episodes of ``ep_len``
    steps, the last one cut at ``M``; ``v_last [L, ceil(M/ep_len)]`` of
    ``v``'s dtype on the GPU bootstraps the episodes' ends (None: they
    are terminal). Arguments the kernel does not take are a
    ``ValueError``."""
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
    if v_last is not None:
        E = -(-M // ep_len)
        if tuple(v_last.shape) != (L, E):
            raise ValueError(
                f"v_last must be [{L}, {E}], got {tuple(v_last.shape)}"
            )
        if v_last.dtype != v.dtype:
            raise ValueError(
                f"v_last must have v's dtype {v.dtype}, got {v_last.dtype}"
            )
        if not v_last.is_cuda:
            raise ValueError("GAE kernel needs its tensors on the GPU")
        v_last = v_last.detach().contiguous().view(-1)
    v = v.detach().contiguous()
    adv = torch.empty_like(v)
    ret = torch.empty_like(v) if want_ret else None
    get_ext().ppo_gae(
        v.view(-1), rews.detach().contiguous().view(-1), stride,
        adv.view(-1), None if ret is None else ret.view(-1), M, ep_len,
        float(gamma), float(lam), v_last,
    )
    return adv, ret
