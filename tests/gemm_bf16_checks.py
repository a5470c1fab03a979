"""Inputs and fp64 references for the bf16-operand linear kernels.

The reference of every contraction is the fp64 product of the
bf16-ROUNDED operands (torch's cast is round-to-nearest-even), so one
comparison checks the fragment map, the tails and the rounding mode,
and proves the bf16 path ran: the native fp32 kernel misses it by
about 2^-9 relative. What is left for the kernel to differ by is fp32
accumulation: inputs are uniform in [-0.5, 0.5], so a K <= 300 term
sum of products (std 1/12 each) has std <= 1.5 and carries about
6e-8 * 1.5 * sqrt(K) ~ 2e-6 of rounding error, 10x under the fp32
atol that tests/test_ops_gpu.py uses for the same shapes.
"""

import torch

ACT = {"none": 0, "relu": 1, "sin_relu": 2, "sigmoid": 3}
TOL = dict(rtol=2e-4, atol=2e-5)  # test_ops_gpu.TOL[torch.float32]
L = 2
SCALE = 1.5  # sin_relu scale


def bf(t):
    return t.bfloat16().double()


def uniform(*shape, dev, amp=0.5):
    return (torch.rand(*shape, device=dev) - 0.5) * (2 * amp)


def weight(theta, off, rows, cols):
    return theta[:, off:off + rows * cols].reshape(L, rows, cols)


ACT_FWD = {
    "relu": torch.relu, "sigmoid": torch.sigmoid,
    "sin_relu": lambda z: torch.relu(torch.sin(SCALE * z)),
}
ACT_BWD = {  # d act / dz from the fp64 pre-activation z and output y
    "relu": lambda z, y: (y > 0).double(),
    "sigmoid": lambda z, y: y * (1 - y),
    "sin_relu": lambda z, y: (torch.sin(SCALE * z) > 0) * SCALE
    * torch.cos(SCALE * z),
}
