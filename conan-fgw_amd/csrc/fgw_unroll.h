// The scaffolding shared by the unrolled FGW backward kernels: k_fgw_acc_pair_bwd (fgw_acc_grad.hip), k_fgw_mixup_bwd_coupling
// (fgw_mixup_grad.hip), k_fgw_pair_bwd (fgw_pair_grad.hip) and k_fgw_bregman_bwd (fgw_bregman_grad.hip).  ONE statement of what they do alike
// and can share without moving a single instruction of theirs: the storage sizing, the line sums and what is built from them, the operands of
// the pair form and their validation.
//
// What is NOT here, although the kernels state it alike: their plain loops over the entries (marginals in, start plan in, record out / in, the
// check output, NaN everywhere, the final rounded write-out) and the reverse walk of FGWMixup's coupling.  A loop that stands in a kernel's
// body is optimised there from the first pass on; moved into a function, even a forced-inline one, it is simplified on its own first and
// arrives in the kernel in another shape.  Each of these was moved, one at a time ("One definition of the shared
// scaffolding"): every one changed the instructions of the kernels it was moved out of, the walk also the registers and scratch of
// k_fgw_acc_pair_bwd<false>, so each kernel keeps its own.  The line sums were a lambda before: a function of their own either way.
//
// Conventions of the family.  One workgroup of UNROLL_NW wavefronts per pair (or coupling).  fp32 in and out, fp64 in between: the gradients of
// the three matrices and the two weight vectors accumulate in fp64 over the whole walk and are rounded to fp32 once.  Every sum has a fixed
// order (lane <-> line, the wavefronts split its entries, partial sums in wavefront order), there are no atomics and nothing is shared between
// workgroups, so a pair's bits do not depend on its batch.  Every loop is bounded by the caller's caps: the counts read from the forward's
// info are clamped, so a corrupt info can neither leave the record nor lengthen a loop.  A weight that is exactly zero marks a node without
// mass: its entries of every plan are exact zeros and constants of the solve, and its rows / columns of every gradient are written as exactly
// 0.  A flagged pair gets NaN in every gradient, as the reference's autograd gives.
//
// Storage (fp64, pitch P = N | 1): NVEC vectors [N], 16 doubles of reduction space where the kernel reduces over the workgroup, and the
// per-wavefront partial sums [NW][N] are always in LDS; five work matrices, 40 bytes per entry, are in LDS while they fit beside the vectors
// (N <= 61 for every kernel of the family), else in the pair's slice of the workspace: the same code, so the same bits, on both paths.  The
// record of the replay and the three matrix accumulators live in the workspace at every size.
//
// The helpers take tid, lane and wave from the kernel: recomputed from threadIdx.x here they are scheduled differently.
#pragma once
#include "fgw_common.h"

namespace {

constexpr int UNROLL_NW = 8;                // wavefronts per workgroup; the LDS limit is fgw_common.h's LDS_LIMIT

// ---- storage sizing -----------------------------------------------------------------------------------------------------------------------
inline size_t unroll_mat_bytes(int N) { return (size_t)N * fgw_pitch(N) * 40; }
// NVEC: the kernel's [N] vectors; RED: whether 16 doubles of reduction space follow them
template <int NVEC, bool RED>
struct UnrollStore {
    __host__ __device__ static size_t vec_bytes(int N) { return ((size_t)((NVEC + UNROLL_NW) * (size_t)N + (RED ? 16 : 0)) * 8 + 15) / 16 * 16; }      // rounded to 16 bytes
    static bool resident(int N) { return vec_bytes(N) + unroll_mat_bytes(N) <= LDS_LIMIT; }
    static bool supported(int N) { return N > 0 && N <= 16384 && vec_bytes(N) <= LDS_LIMIT; }       // (N P and N N stay far inside int)
    static size_t lds_bytes(int N) { return vec_bytes(N) + (resident(N) ? unroll_mat_bytes(N) : 0); }      // the launch's dynamic LDS
    // bytes per pair: what the kernel keeps in the workspace at every size, + the matrices outside LDS, rounded up to 256
    static size_t stride(int N, size_t always) { return al256(always + (resident(N) ? 0 : unroll_mat_bytes(N))); }
};

// ---- the pair form's operands: the head of AccBwdCall, PairBwdCall and BregmanBwdCall -------------------------------------------------------
struct UnrollPairIO {
    const float *M, *A, *B, *a, *b, *X0;    // the cost, the two structures, the weights (null: uniform), the start (null: a b^T)
    const int *info;
    const float *dX, *ddist;                // the cotangents of the plan and of the distance (one may be null)
    float *dM, *dA, *dB, *da, *db, *dX0, *chk;
};

// What the three pair-form entry points refuse alike; `step` is rho / epsilon.  (conan_status of common.h)
inline int unroll_pair_args(const UnrollPairIO &c, int B, int N, const void *workspace, double step, double alpha) {
    if (!c.M || !c.A || !c.B || !c.info || !c.dM || !c.dA || !c.dB || !workspace || B <= 0 || N <= 0) return CONAN_E_BADARG;
    if (!c.dX && !c.ddist) return CONAN_E_BADARG;
    if ((c.da && !c.a) || (c.db && !c.b) || (c.dX0 && !c.X0)) return CONAN_E_BADARG;
    if (!(step > 0.0 && step <= 1.79769313486231570815e308) || !(alpha == alpha)) return CONAN_E_BADARG;
    return CONAN_OK;
}

// ---- workgroup-collective pieces -----------------------------------------------------------------------------------------------------------
// out[l] = sum over the entries e of line l of f(l, e, offset of the entry): rows (col = false) or columns.  Lane <-> line, the wavefronts
// split its entries, then the partial sums in wavefront order.  Ends on a barrier.  (acc_epochs' row / column sums fold the scaling factor and
// the zero-sum flag into the second loop, and k_fgw_pair_bwd's column maxima start from pm[l], not from 0: other arithmetic, their own loops.)
template <class F>
__device__ __forceinline__ void unroll_line_sums(int tid, int lane, int wave, int N, int P, double *pm, bool col, F f, double *out) {
    constexpr int NW = UNROLL_NW, NT = 64 * NW;
    const int sl = col ? 1 : P, se = col ? P : 1;
    for (int l = lane; l < N; l += 64) {
        double s = 0.0;
        for (int e = wave; e < N; e += NW) s += f(l, e, l * sl + e * se);
        pm[wave * N + l] = s;
    }
    __syncthreads();
    for (int l = tid; l < N; l += NT) {
        double s = 0.0;
#pragma unroll
        for (int u = 0; u < NW; ++u) s += pm[u * N + l];
        out[l] = s;
    }
    __syncthreads();
}

// an entry between two nodes with mass
__device__ __forceinline__ bool unroll_live(const double *pa, const double *qb, int i, int j) { return pa[i] > 0.0 && qb[j] > 0.0; }

// sc = Gb q, qv = Gb^T p: what a start a b^T passes on to the weights from its cotangent Gb
__device__ __forceinline__ void unroll_start_sums(int tid, int lane, int wave, int N, int P, double *pm, const double *Gb, const double *pa,
                                                  const double *qb, double *sc, double *qv) {
    unroll_line_sums(tid, lane, wave, N, P, pm, false, [&](int, int e, int o) { return Gb[o] * qb[e]; }, sc);
    unroll_line_sums(tid, lane, wave, N, P, pm, true, [&](int, int e, int o) { return Gb[o] * pa[e]; }, qv);
}

}  // namespace
