/*
 * conan_fgw_hip_mixup_grad.h — exports of libconan_fgw_hip.so for the unrolled gradient of the FGWMixup barycenter, added after
 * conan_fgw_hip.h was frozen at CONAN_FGW_ABI_VERSION 6.  An added export does not change that version; the conventions (device pointers,
 * stream-ordered, caller-provided workspaces, nothing launched on a bad argument) and the error codes are those of conan_fgw_hip.h.  The Python
 * host binds this header's entry points from _lib.EXT_TABLES["conan_fgw_hip_mixup_grad.h"].
 */
#ifndef CONAN_FGW_HIP_MIXUP_GRAD_H
#define CONAN_FGW_HIP_MIXUP_GRAD_H

#include "conan_fgw_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* conan_fgw_mixup_barycenter_fwd (same arguments, same launches, same bits in every output) that also keeps the barycenter's fp64 state:
 * record, (max_iter + 1) * B * (N * N + N * d) * 8 bytes, receives C_t [B,N,N] for t = 0 .. max_iter (after init and after every update),
 * then Y_t [B,N,d] likewise, copied device to device by the driver as T_iter is; no kernel differs.  A molecule that stopped after n outer
 * iterations repeats its state n in the later entries.  CONAN_E_BADARG for a null record and for everything the plain forward refuses. */
int conan_fgw_mixup_barycenter_fwd_record(const float *Ys, const float *Cs, const float *ps, const float *p, const float *lambdas,
                                          const float *init_C, const float *init_Y, int B, int K, int N, int d, const conan_fgw_params *params,
                                          double rho, int epoch, double eps, float *Y, float *C, float *T, float *T_iter, int *info, float *errs,
                                          void *record, void *workspace, void *stream);

/* The gradient of that solve as torch autograd delivers it through the reference's fgw_barycenters_BAPG (barycenter.py:259-390): through the
 * update steps, the feature costs and every epoch of every coupling solve of every outer iteration the forward ran (info[b,0], read on the
 * device and clamped to [0, max_iter]).  Ys, Cs, ps, p, lambdas, B, K, N, d, params, rho, epoch, eps: the forward's arguments; init_Y: the
 * forward's (only whether it is null is used: the states come from the record); info [B,4], record: the forward's outputs.
 * Cotangents, each nullable but not both: dY [B,N,d], dC [B,N,N].  Outputs, fp32, each nullable, each entry rounded once from an fp64 sum in
 * a fixed order (no atomics): dYs [B,K,N,d], dCs [B,K,N,N], dps [B,K,N], dp [B,N], dlambdas [K] (summed over the molecules, b ascending),
 * dinit_C [B,N,N] (the cotangent of the start C_0: init_C, or Cs[:,0] where the forward had no init_C — the caller adds it there), dinit_Y
 * [B,N,d].  Check outputs, nullable: T_chk [B,K,N,N], the replayed plans of each molecule's last outer iteration (the forward's T bit for
 * bit); epochs_chk [max_iter,B,K] int, the epoch count each replayed solve stopped at (0 where the molecule had stopped before).
 * 2 max_iter + 1 launches, descending from max_iter - 1: one workgroup per coupling that replays the solve with the forward's own objective
 * checks from the recorded state, forms the update steps' partials, walks the half-steps in reverse and differentiates the feature cost;
 * one workgroup per molecule that sums the couplings' shares of the state's cotangent and of dp; one last launch that rounds.
 * A node without mass (p_i = 0 or ps_sj = 0) gets exactly 0 in all its entries.  A molecule whose forward raised flags bit 2 (info[b,3])
 * gets NaN in every gradient of its own and, through the sum, in dlambdas; the other molecules are not touched by it.
 * The five fp64 work matrices (40 bytes per entry) are LDS-resident when conan_fgw_mixup_barycenter_bwd_lds_resident(N) (host only: N <= 61),
 * else in the workspace.  Workspace: conan_fgw_mixup_barycenter_bwd_workspace_bytes(B, K, N, d, epoch), the sum of these regions, each rounded
 * up to 256 bytes, in doubles: B N^2 + B N d + B N for the state's cotangent and dp; B K (4 N^2 + 2 N d + 2 N + 1) for the couplings' shares,
 * accumulators, dM and the unclamped feature cost; B K 2 epoch N^2 for the record of the half-steps, reused by every outer iteration (2.2 GB
 * at B K = 1280, N = 33, epoch 100); B K 5 N (N | 1) outside LDS.  0 for a non-positive argument and where the launch is unsupported.
 * CONAN_E_BADARG, before any launch, for a null Ys / Cs / params / info / record / workspace, both cotangents null, dps without ps, dp without
 * p, dlambdas without lambdas, dinit_Y without init_Y, a non-positive B / K / N / d / epoch / max_iter, rho <= 0 or not finite, a NaN eps,
 * fixed_features without init_Y, a loss code outside {0, 1}; CONAN_E_UNSUPPORTED when the vectors alone exceed the LDS (N > 1279). */
int conan_fgw_mixup_barycenter_bwd_lds_resident(int N);
long long conan_fgw_mixup_barycenter_bwd_workspace_bytes(int B, int K, int N, int d, int epoch);
int conan_fgw_mixup_barycenter_bwd(const float *Ys, const float *Cs, const float *ps, const float *p, const float *lambdas, const float *init_Y,
                                   int B, int K, int N, int d, const conan_fgw_params *params, double rho, int epoch, double eps, const int *info,
                                   const void *record, const float *dY, const float *dC, float *dYs, float *dCs, float *dps, float *dp,
                                   float *dlambdas, float *dinit_C, float *dinit_Y, float *T_chk, int *epochs_chk, void *workspace, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* CONAN_FGW_HIP_MIXUP_GRAD_H */
