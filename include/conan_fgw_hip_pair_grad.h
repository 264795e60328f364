/*
 * conan_fgw_hip_pair_grad.h — exports of libconan_fgw_hip.so for the unrolled gradient of the pairwise entropic FGW solve, added after
 * conan_fgw_hip.h was frozen at CONAN_FGW_ABI_VERSION 6.  An added export does not change that version; the conventions (device pointers,
 * stream-ordered, caller-provided workspaces, nothing launched on a bad argument) and the error codes are those of conan_fgw_hip.h.  The Python
 * host binds this header's entry points from _lib.EXT_TABLES["conan_fgw_hip_pair_grad.h"].
 */
#ifndef CONAN_FGW_HIP_PAIR_GRAD_H
#define CONAN_FGW_HIP_PAIR_GRAD_H

#include "conan_fgw_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The gradient through the unrolled iterations of conan_fgw_pair_fwd with solver 0 (PGD) or 1 (PPA), square loss, as torch autograd delivers
 * it through the reference's fgw (bregman.py:70-167 around sinkhorn_log, sinkhorn.py:388-450): ONE launch, one workgroup per pair, that
 * (1) replays in fp64 the outer iterations the forward ran — info[b,0], read on the device and clamped to [0, max_iter] — from G0 or p q^T,
 * recording every iteration's input plan and the Sinkhorn sweeps it ran (decided here by the reference's rule: zero potentials at every call,
 * the marginal error evaluated where ii % 10 == 0, exit below stop_thr; at most num_iter_max), and (2) walks the iterations in reverse, each
 * with the reverse sweeps of its Sinkhorn call.  M, C1, C2, p, q, G0, B, N: the forward's arguments; alpha, epsilon, stop_thr: the solve's
 * parameters in fp64 (the forward's parameter block holds their fp32 roundings); solver 0 / 1; symmetric 1, 0 or -1 (-1: the decision the
 * forward took, info[b,3]); info[B,4]: the forward's output.
 * Cotangents, each nullable but not both: dT[B,N,N] of the returned plan; ddist[B] of fgw_dist (conan_fgw_pair_dist's value, always from the
 * untransposed problem), whose direct partials in M, C1, C2, p, q are added here.  Outputs, fp32, each entry rounded once from an fp64 sum in a
 * fixed order (no atomics): dM, dC1, dC2 [B,N,N]; dp, dq [B,N] or NULL (NULL where p / q is NULL); dG0 [B,N,N] or NULL (NULL where G0 is NULL:
 * the start p q^T then passes its gradient to dp, dq); T_chk [B,N,N] or NULL: the replay's final plan; binfo [B,2] int or NULL: {the replayed
 * sweep total, flags: bit 0 the total differs from info[b,1]; bit 2 the pair's gradients are NaN}.
 * A node without mass (p_i = 0 or q_j = 0) gets exactly 0 in its rows / columns of dM, dC1, dC2, dG0 and in dp_i / dq_j.  A pair whose
 * forward raised flags bit 2, or whose replay meets a non-finite plan entry or, under PPA, an exact zero of an input plan at an entry with
 * mass (the logarithm the reference takes there), gets NaN in every gradient; the other pairs of the batch are not touched by it.
 * The five fp64 work matrices (40 bytes per entry) are LDS-resident when conan_fgw_pair_bwd_lds_resident(N) (host only: N <= 61), else in the
 * workspace.  Workspace: conan_fgw_pair_bwd_workspace_bytes(B, N, max_iter, num_iter_max) = B times ((max_iter + 3) N^2 * 8 for the record
 * of the input plans and the three fp64 accumulators, + (4 num_iter_max + 2) N * 8 for one Sinkhorn call's potentials and reverse factors,
 * + ceil(max_iter / 2) * 8 for the sweep counts, + 5 N (N | 1) * 8 outside LDS, rounded up to 256); 0 for a non-positive argument and where
 * the launch is unsupported.  CONAN_E_BADARG, before any launch, for a null M / C1 / C2 / info / dM / dC1 / dC2 / workspace, both cotangents
 * null, dp without p, dq without q, dG0 without G0, B <= 0, N <= 0, max_iter <= 0, num_iter_max <= 0, epsilon <= 0 or not finite, a NaN alpha
 * or stop_thr, solver outside {0, 1} or symmetric outside {-1, 0, 1}; CONAN_E_UNSUPPORTED when the vectors alone exceed the LDS (N ~ 850). */
int conan_fgw_pair_bwd_lds_resident(int N);
long long conan_fgw_pair_bwd_workspace_bytes(int B, int N, int max_iter, int num_iter_max);
int conan_fgw_pair_bwd(const float *M, const float *C1, const float *C2, const float *p, const float *q, const float *G0, int B, int N,
                       double alpha, double epsilon, int max_iter, int num_iter_max, double stop_thr, int solver, int symmetric,
                       const int *info, const float *dT, const float *ddist, float *dM, float *dC1, float *dC2, float *dp, float *dq,
                       float *dG0, float *T_chk, int *binfo, void *workspace, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* CONAN_FGW_HIP_PAIR_GRAD_H */
