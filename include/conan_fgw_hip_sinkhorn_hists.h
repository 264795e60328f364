/*
 * conan_fgw_hip_sinkhorn_hists.h — exports of libconan_fgw_hip.so for Sinkhorn-Knopp with several target histograms at once (a 2-D b), added
 * after conan_fgw_hip.h was frozen at CONAN_FGW_ABI_VERSION 6.  An added export does not change that version; the conventions (device pointers,
 * stream-ordered, caller-provided workspaces, nothing launched on a bad argument) and the error codes are those of conan_fgw_hip.h.  The Python
 * host binds this header's entry points from _lib.EXT_TABLES["conan_fgw_hip_sinkhorn_hists.h"].
 */
#ifndef CONAN_FGW_HIP_SINKHORN_HISTS_H
#define CONAN_FGW_HIP_SINKHORN_HISTS_H

#include "conan_fgw_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The reference's sinkhorn_knopp with b [n2, H] (sinkhorn.py:207-315): one cost matrix, one source histogram, H target histograms, the H
 * transport costs, ONE stop for all histograms.  B problems per launch, one workgroup per problem; problem p is n1[p] x n2[p] with nh[p]
 * histograms (device-side int32 arrays, each nullable: N1, N2, H) inside the containers M [N1,N2], b [N2,H]; nothing outside its block is read,
 * outputs outside it are zeros.  M: B matrices m_batch_stride floats apart (0: one M shared by the batch); a [B,N1] or NULL (uniform over
 * n1[p]); b [B,N2,H]; warm_u [B,N1,H], warm_v [B,N2,H]: log u, log v to start from, both or neither.  fp32 in and out, fp64 in between:
 * K = exp((double)M / -reg); per sweep V = b / (K^T U), U = 1 / (((1 / a) K) V); a zero entry of K^T U, a NaN or Inf of U or V in ANY histogram
 * restores the previous U, V of ALL histograms and leaves the loop (flags bit 1); at every 10th sweep err = ||V o (K^T U) - b||_F over all
 * n2 nh entries, stop when err < stop_thr (flags bit 0).  reg and stop_thr are doubles: the caller's values, not their fp32 roundings.
 * Outputs: loss [B,H] = sum_ij u_ik K_ij v_jk M_ij; log_u [B,N1,H], log_v [B,N2,H]; info [B,4] int or NULL = {niter (the reference's
 * log["niter"]), flags, checks executed, 0}; errs [B, ceil(num_iter_max / 10)] or NULL (NaN where not executed).
 * Deterministic: no atomics, every sum in a fixed order that depends on n1[p], n2[p], nh[p] alone: a problem gives the same bits alone, in any
 * batch, at any position and in any container.
 *
 * LDS.  The scaling matrices, their previous values, b and 1 / a are LDS-resident:
 *     vector bytes = (16 + N1 + (2 N1 + 3 N2) (H | 1)) * 8 <= 160 KiB,
 * and conan_sinkhorn_hists_max_hists(N1, N2) is the largest H that satisfies it (0: none, or a non-positive size; never above 65535).
 * K [N1, N2 | 1] fp64 is LDS-resident when vector bytes + N1 (N2 | 1) * 8 <= 160 KiB (conan_sinkhorn_hists_lds_resident, host only), else
 * streamed from the workspace.  conan_sinkhorn_hists_workspace_bytes(B, N1, N2, H): 256 when resident, else B times (N1 (N2 | 1) * 8 rounded
 * up to 256); 0 for a non-positive argument and for an unsupported (N1, N2, H).
 * CONAN_E_BADARG, before any launch, for a null M / b / loss / log_u / log_v / workspace, one warm start without the other, B, N1, N2, H or
 * num_iter_max <= 0, m_batch_stride < 0, reg <= 0 or not finite, a NaN stop_thr; CONAN_E_UNSUPPORTED, never launched, for H above
 * conan_sinkhorn_hists_max_hists(N1, N2). */
int conan_sinkhorn_hists_max_hists(int N1, int N2);
int conan_sinkhorn_hists_lds_resident(int N1, int N2, int H);
long long conan_sinkhorn_hists_workspace_bytes(int B, int N1, int N2, int H);
int conan_sinkhorn_hists_fwd(const float *M, const float *a, const float *b, const float *warm_u, const float *warm_v, const int *n1, const int *n2,
                             const int *nh, int B, int N1, int N2, int H, long long m_batch_stride, double reg, int num_iter_max, double stop_thr,
                             float *loss, float *log_u, float *log_v, int *info, float *errs, void *workspace, void *stream);

/* The fixed-plan gradient of those costs to M: dM[p,i,j] = K_ij sum_k g[p,k] u_ik v_jk with K recomputed from M and u, v from the forward's
 * log_u, log_v; g [B,H] the cotangent of loss; dM [B,N1,N2], zeros outside the problem's block.  One workgroup per problem, no workspace, no
 * [H,N1,N2] tensor.  CONAN_E_BADARG for a null pointer among M, log_u, log_v, g, dM, a non-positive size, m_batch_stride < 0, reg <= 0 or not
 * finite; CONAN_E_UNSUPPORTED as the forward. */
int conan_sinkhorn_hists_loss_bwd(const float *M, const float *log_u, const float *log_v, const float *g, const int *n1, const int *n2, const int *nh,
                                  int B, int N1, int N2, int H, long long m_batch_stride, double reg, float *dM, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* CONAN_FGW_HIP_SINKHORN_HISTS_H */
