// The epochs of FGWMixup's coupling solve (the reference's fused_ACC_torch, barycenter.py:228-256), ONE statement for everything that runs them:
// the two forward kernels of fgw_acc.hip and the replay of the unrolled gradient (fgw_acc_grad.hip), which has to retrace the forward's iterates
// bit for bit.  The file comment of fgw_acc.hip describes the iteration.
#pragma once
#include "fgw_unroll.h"

namespace {

constexpr int ACC_NW = UNROLL_NW;           // (the replay hands acc_epochs the backward's pm: one wavefront count for both)
constexpr size_t ACC_LDS_LIMIT = LDS_LIMIT;

// vectors: a, b, the scaling factors, |y_i|^2, |z_j|^2 [N] each, 16 doubles of reduction space, per-wavefront partial sums [NW][N]; rounded to 16 bytes
__host__ __device__ inline size_t acc_vec_bytes(int N) { return ((size_t)((5 + ACC_NW) * N + 16) * 8 + 15) / 16 * 16; }
inline size_t acc_lds(int N) { return acc_vec_bytes(N) + (size_t)N * fgw_pitch(N) * 24; }

// What one coupling solve reads and writes beyond the matrices' storage.
template <typename TA>
struct AccProblem {
    const TA *A;              // [N,N]: the barycenter structure (fp64 state) or the pair's A
    const float *Bm;          // [N,N]: the input graph's structure, untransposed
    double alpha, rho, eps;
    int epoch;
    float *objs;              // pair form: [nobj] objective of every check (the caller filled it with NaN); else null
};
struct AccResult {
    int epochs, stored, zero_sum;
};

// The hook of acc_epochs: rec(h, X) is called by every thread with the input of half-step h = 2 ii + ph (ph 0: the row step, after the 1e-10
// lift; ph 1: the column step) while X is at rest between two barriers.  It may read X and write memory of its own; the forward passes none.
struct AccNoRecord {
    __device__ __forceinline__ void operator()(int, const double *) const {}
};

// The epochs.  pa / qb (the marginals), X (the start) and Mb are in place; AX, sc, pm, red are work space.  Workgroup-collective; every value
// that steers the loop comes out of block_sum_d and is the same in every thread.  CHECKS = false (the replay): no objective is formed and
// nothing stops the loop, exactly q.epoch epochs run; the half-steps are the same instructions either way.
template <bool CHECKS = true, typename TA, class REC = AccNoRecord>
__device__ __forceinline__ AccResult acc_epochs(const AccProblem<TA> &q, int N, int P, const double *pa, const double *qb, double *sc, double *pm,
                                                double *red, double *X, double *AX, const double *Mb, REC rec = REC{}) {
    constexpr int NW = ACC_NW, NT = 64 * NW;
    const int NN = N * N;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const double four_alpha = 4.0 * q.alpha, two_alpha = 2.0 * q.alpha, inv_rho = 1.0 / q.rho;

    auto bad_sum = [](double s) { return !(s > 0.0 && s <= 1.79769313486231570815e308); };

    AccResult r{q.epoch, 0, 0};
    double last = 0.0;
    bool stop = false;
    for (int ii = 0; ii < q.epoch && !stop; ++ii) {
        for (int t = tid; t < NN; t += NT) {
            const int i = t / N, j = t - i * N;
            if (pa[i] > 0.0 && qb[j] > 0.0) X[i * P + j] += 1e-10;
        }
        __syncthreads();
        // phase 0: the row half-step, 1: the column half-step, 2: the objective (every 10th epoch from the 11th on).  One text for the two
        // products of all three: G = (A X) B, consumed entry by entry as it leaves the matrix pipe.
        const int phases = (CHECKS && ii > 0 && ii % 10 == 0) ? 3 : 2;
        for (int ph = 0; ph < phases; ++ph) {
            if (ph < 2) rec(2 * ii + ph, X);
            mm_f64_glb<NW, false>(N, N, N, q.A, N, X, P, [&](int i, int j, double v) { AX[i * P + j] = v; });
            __syncthreads();
            double part = 0.0;
            mm_f64_glb<NW, false>(N, N, N, AX, P, q.Bm, N, [&](int i, int j, double g) {
                const double x = X[i * P + j], m = Mb[i * P + j];
                if (ph == 2) { part += (m - two_alpha * g) * x; return; }
                // X <- X * exp((4 alpha (A X) B - Mb) / rho) in place (this product reads AX, not X); massless rows / columns stay exactly zero
                X[i * P + j] = (pa[i] > 0.0 && qb[j] > 0.0) ? x * exp((four_alpha * g - m) * inv_rho) : 0.0;
            });
            if (ph == 2) {
                const double obj = block_sum_d<NW>(part, red);
                if (q.objs && tid == 0) q.objs[ii / 10 - 1] = (float)obj;
                if (r.stored > 0 && fabs((obj - last) / last) < q.eps) { r.epochs = ii + 1; stop = true; }      // (a NaN compares false: stored, the loop goes on)
                else { last = obj; ++r.stored; }
                break;
            }
            __syncthreads();
            // X <- diag(a / rowsum X) X (ph 0) or X diag(b / colsum X) (ph 1): lane <-> the summed line, the wavefronts split its entries
            const double *w = ph ? qb : pa;
            const int sl = ph ? 1 : P, se = ph ? P : 1;
            for (int i = lane; i < N; i += 64) {
                double sum = 0.0;
                for (int j = wave; j < N; j += NW) sum += X[i * sl + j * se];
                pm[wave * N + i] = sum;
            }
            __syncthreads();
            for (int i = tid; i < N; i += NT) {
                double sum = 0.0;
#pragma unroll
                for (int u = 0; u < NW; ++u) sum += pm[u * N + i];
                if (w[i] > 0.0 && bad_sum(sum)) r.zero_sum = 1;
                sc[i] = w[i] > 0.0 ? w[i] / sum : 0.0;                  // a_i / 0: the reference's NaN (inf * 0) follows
            }
            __syncthreads();
            for (int t = tid; t < NN; t += NT) { const int i = t / N, j = t - i * N; X[i * P + j] *= sc[ph ? j : i]; }
            __syncthreads();
        }
    }
    r.zero_sum = block_sum_d<NW>((double)r.zero_sum, red) > 0.0 ? 1 : 0;
    return r;
}

// carve of the dynamic LDS (and, outside LDS, of the coupling's scratch slice)
struct AccCarve {
    double *pa, *qb, *sc, *y2a, *z2a, *red, *pm, *X, *AX, *Mb;
};
template <bool LDS>
__device__ __forceinline__ AccCarve acc_carve(char *smem, int N, int P, char *slice) {
    AccCarve c;
    c.pa = reinterpret_cast<double *>(smem); c.qb = c.pa + N; c.sc = c.pa + 2 * N; c.y2a = c.pa + 3 * N; c.z2a = c.pa + 4 * N;
    c.red = c.pa + 5 * N; c.pm = c.red + 16;
    c.X = reinterpret_cast<double *>(LDS ? smem + acc_vec_bytes(N) : slice); c.AX = c.X + N * P; c.Mb = c.AX + N * P;
    return c;
}

}  // namespace
