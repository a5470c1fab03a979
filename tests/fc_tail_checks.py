"""Cases and runner for test_fc_tail_mfma_gpu.py.

Which fc kernel ext.fc_block runs on is fixed per process
(NDTA_FC_SPLIT=0: fc_block_k, 1: fc_fwd_split_k + fc_dx0_k), so the test
starts this file once per setting:

    python fc_tail_checks.py OUT.pt

runs every case below in order, in fp64 and fp32, and saves the inputs
and the outputs (CPU tensors) to OUT.pt.
"""

import sys

import torch

from test_fc_split_gpu import LOSS_SCALE, OFF, _inputs, _offsets

SENTINEL = -77.0

# name -> (L, M, I, H, C, x0 scale). The fc2 tail works on a [16 m]
# x [16 c] x [64 h] tile whatever M, C and H are; I only feeds fc1, so it
# is as small as a 16-column dX0 strip plus a tail allows.
CASES = {
    # pad classes: C = 16 has none, 1 is a softmax over one class
    "C10": (2, 16, 24, 64, 10, 1.0),
    "C16": (2, 16, 24, 64, 16, 1.0),
    "C3": (2, 16, 24, 64, 3, 1.0),
    "C1": (2, 16, 24, 64, 1, 1.0),
    # pad columns of W2 / y1, the h < H guards; 8 leaves 3 of the 4
    # h-fragments all padding
    "H32": (2, 16, 24, 32, 10, 1.0),
    "H8": (2, 16, 24, 8, 10, 1.0),
    # row tails: one row, a second tile of one row, of four
    "M1": (2, 1, 24, 64, 10, 1.0),
    "M17": (2, 17, 24, 64, 10, 1.0),
    "M20": (2, 20, 24, 64, 10, 1.0),
    # dirty LDS: activations near 1e3 in all 64 columns and all 16
    # classes, then (next in this process) a case that uses 8 columns
    # and 3 classes of the same arenas
    "big": (2, 16, 24, 64, 16, 1e3),
    "after_big": (2, 16, 24, 8, 3, 1.0),
    # one row per node: each node's loss is a single atomicAdd
    "rows1": (20, 1, 24, 64, 10, 1.0),
}
# run twice on the same inputs (order of the logit partial sums)
TWICE = ("M20", "rows1")
DTYPES = {"fp64": torch.float64, "fp32": torch.float32}


def case_inputs(name, dtype):
    L, M, I, H, C, scale = CASES[name]
    theta, x0, Y_all, idx, maxlen = _inputs(41, dtype, L, M, I, H, C, True)
    return theta, x0 * scale, Y_all, idx, maxlen


def call(ext, inp, M, I, H, C):
    """ext.fc_block with one sentinel row behind dz1g."""
    theta, x0, Y_all, idx, maxlen = inp
    L = theta.shape[0]
    w1, b1, w2, b2, _ = _offsets(I, H, C)
    grad = torch.zeros_like(theta)
    dx0 = torch.empty_like(x0)
    buf = torch.full((L * M + 1, H), SENTINEL, dtype=x0.dtype,
                     device=x0.device)
    loss = torch.zeros(L, dtype=x0.dtype, device=x0.device)
    ext.fc_block(x0, theta, Y_all, idx, maxlen, OFF, grad, dx0,
                 buf[:L * M], loss, w1, b1, w2, b2, M, I, H, C,
                 LOSS_SCALE, True)
    return dict(grad=grad, dx0=dx0, dz1=buf[:L * M], guard=buf[L * M],
                loss=loss)


def main(out_path):
    from nn_distributed_training_amd.ops import get_ext

    ext = get_ext()
    res = {}
    for name, (L, M, I, H, C, _) in CASES.items():
        for dname, dtype in DTYPES.items():
            inp = case_inputs(name, dtype)
            outs = [call(ext, inp, M, I, H, C)
                    for _ in range(2 if name in TWICE else 1)]
            torch.cuda.synchronize()
            res[name, dname] = dict(
                inp=tuple(t.cpu() if torch.is_tensor(t) else t
                          for t in inp),
                outs=[{k: v.cpu() for k, v in o.items()} for o in outs])
    torch.save(res, out_path)


if __name__ == "__main__":
    main(sys.argv[1])
