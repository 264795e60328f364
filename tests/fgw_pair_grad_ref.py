"""The reference expression of the pair distance for the gradient tests (test infrastructure): fgw_dist of bregman.py:163-164 with init_matrix /
gwloss of utils.py:4-59 restated in torch for a batch, to be differentiated by torch autograd in fp64 at a fixed plan.  test_fgw_pair_grad_cpu.py
pins it to the reference's own gradients (tests/golden/fgw_distgrad_*.npz); the GPU tests use it where there is no fixture."""
import torch


def fgw_dist_torch(M, C1, C2, p, q, T, alpha, loss_fun="square_loss"):
    """M, T [B,n1,n2], C1 [B,n1,n1], C2 [B,n2,n2], p [B,n1], q [B,n2] -> [B]."""
    if loss_fun == "square_loss":
        f1, f2, h2 = C1 * C1, C2 * C2, 2 * C2
    else:
        f1, f2, h2 = C1 * torch.log(C1 + 1e-15) - C1, C2, torch.log(C2 + 1e-15)
    constC = (f1 @ p[:, :, None]) + (f2 @ q[:, :, None]).transpose(1, 2)          # constC_ij = sum_k f1(C1_ik) p_k + sum_k q_k f2(C2_jk)
    tens = constC - C1 @ T @ h2.transpose(1, 2)
    return (1 - alpha) * (M * T).sum((1, 2)) + alpha * (tens * T).sum((1, 2))


def fgw_dist_grads(M, C1, C2, p, q, T, alpha, loss_fun="square_loss", gout=None):
    """The gradients of sum_b gout[b] fgw_dist_torch(...)[b] in (M, C1, C2, p, q), formed in fp64 whatever the inputs' dtype; T is a constant."""
    leaves = [x.detach().double().requires_grad_(True) for x in (M, C1, C2, p, q)]
    d = fgw_dist_torch(*leaves, T.detach().double(), alpha, loss_fun)
    return torch.autograd.grad(d.sum() if gout is None else (d * gout.double()).sum(), leaves)
