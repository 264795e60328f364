/*
 * conan_fgw_hip_ext.h — exports of libconan_fgw_hip.so added after conan_fgw_hip.h was frozen at CONAN_FGW_ABI_VERSION 6.  An added export does
 * not change that version; the conventions (device pointers, stream-ordered, caller-provided workspaces, nothing launched on a bad argument) and
 * the error codes are those of conan_fgw_hip.h.  The Python host binds this header's entry points from _lib.EXT_SIGNATURES.
 */
#ifndef CONAN_FGW_HIP_EXT_H
#define CONAN_FGW_HIP_EXT_H

#include "conan_fgw_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The gradient through the unrolled epochs of conan_fgw_acc_pair_fwd, as torch autograd delivers it through the reference's fused_ACC_torch
 * (barycenter.py:228-256): ONE launch, one workgroup per pair, that (1) replays the epochs the forward ran — info[b,0], read on the device and
 * clamped to [0, epoch]; the forward's own loop without the objective checks — recording the fp64 input of every half-step in the workspace, and
 * (2) walks the half-steps in reverse.  M, A, Bm, a, b, X0, B, N, alpha, rho, epoch: the forward's arguments; info[B,4]: the forward's output.
 * Cotangents, each nullable but not both: dX[B,N,N] of the returned plan; ddist[B] of the FGWMixup distance of that plan,
 *   (1 - alpha) <M, X> + alpha (<c1, X> - 2 <A X Bm, X>),   c1 = (A o A) a 1^T + 1 b^T (Bm o Bm)
 * (conan_fgw_pair_dist with C2 = Bm^T), whose direct partials in M, A, Bm, a, b are added here.  Outputs, fp32, each entry rounded once from an
 * fp64 sum in a fixed order (no atomics): dM, dA, dBm [B,N,N]; da, db [B,N] or NULL (NULL where a / b is NULL); dX0 [B,N,N] or NULL (NULL
 * where X0 is NULL: the start a b^T then passes its gradient to da, db); X_chk [B,N,N] or NULL: the replay's final X, the forward's bit for bit.
 * A node without mass (a_i = 0 or b_j = 0) gets exactly 0 in its rows / columns of dM, dA, dBm, dX0 and in da_i / db_j; a pair whose forward
 * raised flags bit 2 gets NaN in every gradient.
 * The five fp64 work matrices (40 bytes per entry) are LDS-resident when conan_fgw_acc_pair_bwd_lds_resident(N) (host only: N <= 61), else in
 * the workspace.  Workspace: conan_fgw_acc_pair_bwd_workspace_bytes(B, N, epoch) = B times ((2 epoch + 3) N^2 * 8, + 5 N (N | 1) * 8 outside
 * LDS, rounded up to 256): the record of the half-steps' inputs is B * 2 epoch * N^2 * 8 bytes of it (3.5 MB per 33 x 33 pair at epoch = 200);
 * 0 for a non-positive B, N or epoch and where the launch is unsupported.  CONAN_E_BADARG, before any launch, for a null M / A / Bm / info / dM /
 * dA / dBm / workspace, both cotangents null, da without a, db without b, dX0 without X0, B <= 0, N <= 0, epoch <= 0, rho <= 0 or not finite,
 * or a NaN alpha; CONAN_E_UNSUPPORTED when the vectors alone exceed the LDS (N ~ 1270). */
int conan_fgw_acc_pair_bwd_lds_resident(int N);
long long conan_fgw_acc_pair_bwd_workspace_bytes(int B, int N, int epoch);
int conan_fgw_acc_pair_bwd(const float *M, const float *A, const float *Bm, const float *a, const float *b, const float *X0, int B, int N,
                           double alpha, double rho, int epoch, const int *info, const float *dX, const float *ddist,
                           float *dM, float *dA, float *dBm, float *da, float *db, float *dX0, float *X_chk, void *workspace, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* CONAN_FGW_HIP_EXT_H */
