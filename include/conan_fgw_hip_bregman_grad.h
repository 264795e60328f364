/*
 * conan_fgw_hip_bregman_grad.h — exports of libconan_fgw_hip.so for the unrolled gradient of the pairwise BAPG FGW solve, added after
 * conan_fgw_hip.h was frozen at CONAN_FGW_ABI_VERSION 6.  An added export does not change that version; the conventions (device pointers,
 * stream-ordered, caller-provided workspaces, nothing launched on a bad argument) and the error codes are those of conan_fgw_hip.h.  The Python
 * host binds this header's entry points from _lib.EXT_TABLES["conan_fgw_hip_bregman_grad.h"].
 */
#ifndef CONAN_FGW_HIP_BREGMAN_GRAD_H
#define CONAN_FGW_HIP_BREGMAN_GRAD_H

#include "conan_fgw_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The gradient through the unrolled Bregman half-steps of conan_fgw_pair_fwd with solver 2 (BAPG), square or kl loss, as torch autograd delivers
 * it through the reference's fgw_bregman (bregman.py:170-279): ONE launch, one workgroup per pair, that (1) replays in fp64 the iterations the
 * forward ran — info[b,0], read on the device and clamped to [0, max_iter]; never re-decided — from G0 or p q^T, recording the input plan of
 * every half-step (two per iteration), and (2) walks the half-steps in reverse.  M, C1, C2, p, q, G0, B, N: the forward's arguments; alpha,
 * epsilon: the solve's parameters in fp64 (the forward's parameter block holds their fp32 roundings); loss_fun 0 (square) or 1 (kl);
 * symmetric 1, 0 or -1 (-1: the decision the forward took, info[b,3]); info[B,4]: the forward's output.
 * Cotangents, each nullable but not both: dT[B,N,N] of the returned plan; ddist[B] of fgw_dist (conan_fgw_pair_dist's value, always from the
 * untransposed problem), whose direct partials in M, C1, C2, p, q are added here.  Outputs, fp32, each entry rounded once from an fp64 sum in a
 * fixed order (no atomics): dM, dC1, dC2 [B,N,N]; dp, dq [B,N] or NULL (NULL where p / q is NULL); dG0 [B,N,N] or NULL (NULL where G0 is NULL:
 * the start p q^T then passes its gradient to dp, dq); T_chk [B,N,N] or NULL: the replay's final plan; binfo [B,2] int or NULL: {the replayed
 * iteration count, flags: bit 2 the pair's gradients are NaN}.
 * A node without mass (p_i = 0 or q_j = 0) gets exactly 0 in its rows / columns of dM, dC1, dC2, dG0 and in dp_i / dq_j.  A pair whose
 * forward raised flags bit 2, or whose replay meets a zero sum on a node with mass or a non-finite plan entry, gets NaN in every gradient; the
 * other pairs of the batch are not touched by it.
 * The five fp64 work matrices (40 bytes per entry) are LDS-resident when conan_fgw_bregman_bwd_lds_resident(N) (host only: N <= 61), else in the
 * workspace.  Workspace: conan_fgw_bregman_bwd_workspace_bytes(B, N, max_iter) = B times ((2 max_iter + 4) N^2 * 8 for the record of the
 * half-steps' input plans, the three fp64 accumulators and h(C2), + 5 N (N | 1) * 8 outside LDS, rounded up to 256); 0 for a non-positive
 * argument and where the launch is unsupported.  CONAN_E_BADARG, before any launch, for a null M / C1 / C2 / info / dM / dC1 / dC2 /
 * workspace, both cotangents null, dp without p, dq without q, dG0 without G0, B <= 0, N <= 0, max_iter <= 0, epsilon <= 0 or not finite, a
 * NaN alpha, loss_fun outside {0, 1} or symmetric outside {-1, 0, 1}; CONAN_E_UNSUPPORTED when the vectors alone exceed the LDS (N ~ 1070). */
int conan_fgw_bregman_bwd_lds_resident(int N);
long long conan_fgw_bregman_bwd_workspace_bytes(int B, int N, int max_iter);
int conan_fgw_bregman_bwd(const float *M, const float *C1, const float *C2, const float *p, const float *q, const float *G0, int B, int N,
                          double alpha, double epsilon, int max_iter, int loss_fun, int symmetric, const int *info, const float *dT,
                          const float *ddist, float *dM, float *dC1, float *dC2, float *dp, float *dq, float *dG0, float *T_chk, int *binfo,
                          void *workspace, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* CONAN_FGW_HIP_BREGMAN_GRAD_H */
