"""Child process of tests/test_bwd_step_gpu.py::test_driver_rounds.

    python bwd_step_checks.py OUT.pt

Three DiNNO rounds of the stacked driver on a ring of four MNIST nodes
(batch 16, fp64, two primal iterations) from the fixed state of
test_step_dual_gpu._driver. NDTA_BWD_STEP is read once per process by
the native dispatch, which is why each setting runs in a process of its
own. Saves theta, duals and what the dispatch said.
"""

import sys

import torch

from test_step_dual_gpu import _driver

ROUNDS = 3
N = 4


def main(out_path):
    torch.set_default_dtype(torch.float64)
    drv = _driver(N)
    eng = drv.eng
    conv, fc1, _ = eng.spec.layers
    fused = eng.ext.bwd_step_fused_for(
        N, eng.B, fc1.in_dim, fc1.out_dim, conv.out_dim, conv.kernel_size,
        conv.in_dim, 8, 1)
    theta_obj = eng.theta
    same = True
    for k in range(ROUNDS):
        drv.step_round(k)
        same = same and eng.theta is theta_obj
    torch.cuda.synchronize()
    torch.save(
        {"theta": eng.theta.cpu(), "duals": drv.duals.cpu(),
         "fused": fused, "same_theta_object": same,
         "grad_zero": bool((eng.grad == 0).all())},
        out_path)


if __name__ == "__main__":
    main(sys.argv[1])
