// The other three solvers of the reference's sinkhorn dispatcher for gfx950, B problems per launch, one workgroup per problem
// (conan_sinkhorn_ext_fwd; DESIGN.md 3.3, "Sinkhorn: the remaining solvers"):
//     method 2  greenkhorn                 (sinkhorn.py:453-532)   k_greenkhorn      one wavefront per problem
//     method 3  sinkhorn_stabilized        (:535-685, 1-D b)       k_sinkhorn_stab   SX_NW wavefronts per problem
//     method 4  sinkhorn_epsilon_scaling   (:688-786)              k_sinkhorn_stab   the outer loop around the same body, inside the launch
// Conventions as k_sinkhorn (sinkhorn.hip): problem b is n1[b] x n2[b] inside an [N1, N2] container, its matrix has the problem's own pitch
// P = n2[b] | 1, zeros are written outside its block; fp32 in and out (the potentials alpha, beta and the warm start: fp64), fp64 in between; every sum in a fixed order that depends on the problem's
// own sizes alone (per lane in index order, the xor butterfly over the 64 lanes, the wavefronts in order), no atomics, nothing shared between
// workgroups, every loop bounded by the iteration arguments.  K lives in LDS when the container fits (conan_sinkhorn_ext_lds_resident), else in the
// problem's slice of the workspace; the eight vectors are always in LDS.
//
// The control flow is the reference's, decided on fp64 values.
// Stabilized: K = exp(-(M - alpha_i - beta_j) / reg) (M re-read as fp32 at every rebuild), sweep v = b / (K^T u), u = a / (K v); absorption when
// max|u| > tau or max|v| > tau (the maxima carry NaN as torch.max does: they are taken on bit patterns, and a NaN compares false); check at
// ii % print_period == 0 on Gamma(alpha, beta, u, v) AFTER a possible absorption; stop on err <= stop_thr; then the NaN exit (previous u, v).
// Epsilon scaling: reg_i = (epsilon0 - reg) e^-i + reg, inner solves with print_period 20 warm-started from (alpha, beta), which then become
// alpha + reg_i log u, beta + reg_i log v; every print_period outer iterations err = ||colsum G - b||^2 + ||rowsum G - a||^2; leave on
// err <= stop_thr and ii > 35.
// Greenkhorn: K = exp(-M / reg), viol = rowsum(u K v) - a, viol_2 = colsum(u K v) - b; per step the arg-max of |viol| and of |viol_2| (lowest
// index on a tie), the row when the first maximum is strictly larger, else the column, the reference's incremental updates of viol / viol_2,
// and the break after the update when the larger maximum is <= stop_thr.  A step is a latency chain of two arg-max reductions, one dot product
// and one axpy: one wavefront runs it without waiting for anybody.
#include "fgw_common.h"
namespace {
constexpr int SX_NW = 4, SX_NT = 64 * SX_NW;
typedef unsigned long long sx_u64;
constexpr sx_u64 SX_INF_BITS = 0x7ff0000000000000ull, SX_ABS_MASK = 0x7fffffffffffffffull;

struct SxCall {
    const float *M, *a, *b;
    const double *wu, *wv;         // fp64: the potentials of epsilon scaling carry an offset of ~epsilon0 log n, which fp32 resolves to 2e-3 only
    const int *n1, *n2;
    int N1, N2, method, num_iter_max, nerr, print_period, num_inner;
    long long m_stride;
    double reg, stop_thr, tau, eps0;
    float *T, *loss, *log_u, *log_v, *errs;
    double *alpha, *beta;
    int *info, *extra;
    double *ws;
    size_t ws_stride;              // doubles per problem
};

inline size_t sx_vec_bytes(int N1, int N2) { return (size_t)(16 + 4 * (size_t)N1 + 4 * (size_t)N2) * 8; }
inline size_t sx_mat_bytes(int N1, int N2) { return (size_t)N1 * (size_t)(N2 | 1) * 8; }

// torch.full((n,), 1.0 / n).to(M): the reference's uniform vectors (default marginals, initial and reset scalings) are fp32 values
__device__ __forceinline__ double sx_uniform(int n) { return (double)(float)(1.0 / (double)n); }
__device__ __forceinline__ sx_u64 sx_absbits(double x) { return (sx_u64)__double_as_longlong(x) & SX_ABS_MASK; }
__device__ __forceinline__ sx_u64 sx_wave_max_bits(sx_u64 v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { const sx_u64 w = __shfl_xor(v, o, 64); v = w > v ? w : v; }
    return v;
}

// The views of one problem: red (16 doubles; slots 4..7 / 8..11 the wavefronts' maxima of |u| / |v|), a, alpha, two u, b, beta, two v, K.
struct SxS {
    double *red, *av, *al, *u0, *u1, *bv, *be, *v0, *v1, *K;
    const float *M;
    int m1, m2, P, N2;
};

// outputs outside the problem's block; returns true for an empty problem (workgroup-uniform)
template <int NT>
__device__ __forceinline__ bool sx_padding(const SxCall &c, int b, int m1, int m2, int tid) {
    const int N1 = c.N1, N2 = c.N2;
    float *T = c.T + (size_t)b * N1 * N2;
    for (int t = tid; t < N1 * N2; t += NT) {
        const int i = t / N2, j = t - i * N2;
        if (i >= m1 || j >= m2) T[t] = 0.f;
    }
    for (int i = m1 + tid; i < N1; i += NT) {
        if (c.log_u) c.log_u[(size_t)b * N1 + i] = 0.f;
        if (c.alpha) c.alpha[(size_t)b * N1 + i] = 0.0;
    }
    for (int j = m2 + tid; j < N2; j += NT) {
        if (c.log_v) c.log_v[(size_t)b * N2 + j] = 0.f;
        if (c.beta) c.beta[(size_t)b * N2 + j] = 0.0;
    }
    if (c.errs) for (int t = tid; t < c.nerr; t += NT) c.errs[(size_t)b * c.nerr + t] = __builtin_nanf("");
    if (m1 > 0 && m2 > 0) return false;
    if (c.info && tid < 4) c.info[b * 4 + tid] = 0;
    if (c.extra && tid < 4) c.extra[b * 4 + tid] = 0;
    if (c.loss && tid == 0) c.loss[b] = 0.f;
    return true;
}

__device__ __forceinline__ SxS sx_views(const SxCall &c, char *smem, bool resident, int b, int m1, int m2) {
    SxS s;
    const int N1 = c.N1, N2 = c.N2;
    s.red = reinterpret_cast<double *>(smem);
    s.av = s.red + 16; s.al = s.av + N1; s.u0 = s.al + N1; s.u1 = s.u0 + N1;
    s.bv = s.u1 + N1; s.be = s.bv + N2; s.v0 = s.be + N2; s.v1 = s.v0 + N2;
    s.K = resident ? s.v1 + N2 : c.ws + (size_t)b * c.ws_stride;
    s.M = c.M + (size_t)b * (size_t)c.m_stride;
    s.m1 = m1; s.m2 = m2; s.P = m2 | 1; s.N2 = N2;
    return s;
}

// log Gamma_ij of the reference's get_Gamma, in its order of operations; lu, lv hold log u, log v
__device__ __forceinline__ double sx_gamma(const SxS &s, double reg, const double *lu, const double *lv, int i, int j) {
    return exp(-(((double)s.M[(size_t)i * s.N2 + j] - s.al[i]) - s.be[j]) / reg + lu[i] + lv[j]);
}

__device__ __forceinline__ void sx_build_K(const SxS &s, double reg, int tid) {
    const int mm = s.m1 * s.m2;
    for (int t = tid; t < mm; t += SX_NT) {
        const int i = t / s.m2, j = t - i * s.m2;
        s.K[i * s.P + j] = exp(-(((double)s.M[(size_t)i * s.N2 + j] - s.al[i]) - s.be[j]) / reg);
    }
}

// One stabilized solve (sinkhorn.py:535-685) from the potentials in s.al / s.be.  INNER: an inner solve of epsilon scaling, which keeps no error
// list.  On return the current u, v are in buffer pair `cur`, the other pair is free.  Returns the reference's n_iter (the loop index at exit);
// flags bit 0: stopped on err <= thr, bit 1: the NaN exit.  Workgroup-collective; every branch below is workgroup-uniform.
template <bool INNER>
__device__ int sx_stabilized(const SxS &s, double reg, int itmax, double thr, double tau, int pp, float *errs, int &cur, int &flags, int &nchk,
                             int &nabs) {
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int m1 = s.m1, m2 = s.m2, P = s.P;
    const double *K = s.K;
    sx_u64 *redb = reinterpret_cast<sx_u64 *>(s.red);
    const double iu = sx_uniform(m1), iv = sx_uniform(m2);
    __syncthreads();
    for (int i = tid; i < m1; i += SX_NT) s.u0[i] = iu;
    for (int j = tid; j < m2; j += SX_NT) s.v0[j] = iv;
    sx_build_K(s, reg, tid);
    __syncthreads();
    cur = 0; flags = 0;
    int ii = 0;
    for (; ii < itmax; ++ii) {
        double *uo = cur ? s.u1 : s.u0, *vo = cur ? s.v1 : s.v0;
        double *un = cur ? s.u0 : s.u1, *vn = cur ? s.v0 : s.v1;
        sx_u64 mv = 0, mu = 0;
        for (int j = wave; j < m2; j += SX_NW) {                          // v = b / (K^T u)                                      (sinkhorn.py:604)
            double sum = 0.0;
            for (int i = lane; i < m1; i += 64) sum += K[i * P + j] * uo[i];
            sum = wave_sum_d(sum);
            const double vj = s.bv[j] / sum;
            if (lane == 0) vn[j] = vj;
            const sx_u64 k = sx_absbits(vj);
            mv = k > mv ? k : mv;
        }
        __syncthreads();
        for (int i = wave; i < m1; i += SX_NW) {                          // u = a / (K v)                                        (:605)
            double sum = 0.0;
            for (int j = lane; j < m2; j += 64) sum += K[i * P + j] * vn[j];
            sum = wave_sum_d(sum);
            const double ui = s.av[i] / sum;
            if (lane == 0) un[i] = ui;
            const sx_u64 k = sx_absbits(ui);
            mu = k > mu ? k : mu;
        }
        if (lane == 0) { redb[4 + wave] = mu; redb[8 + wave] = mv; }
        __syncthreads();
        sx_u64 MU = redb[4], MV = redb[8];
#pragma unroll
        for (int w = 1; w < SX_NW; ++w) { MU = redb[4 + w] > MU ? redb[4 + w] : MU; MV = redb[8 + w] > MV ? redb[8 + w] : MV; }
        // (the slots are written again only after the next sweep's first barrier)
        const bool absorb = __longlong_as_double((long long)MU) > tau || __longlong_as_double((long long)MV) > tau;      // a NaN maximum compares false (:608)
        bool nan = false;
        if (absorb) {                                                     // alpha += reg log u, beta += reg log v, u = 1 / n1, v = 1 / n2, K rebuilt    (:614-621)
            for (int i = tid; i < m1; i += SX_NT) { s.al[i] = s.al[i] + reg * log(un[i]); un[i] = iu; }
            for (int j = tid; j < m2; j += SX_NT) { s.be[j] = s.be[j] + reg * log(vn[j]); vn[j] = iv; }
            __syncthreads();
            sx_build_K(s, reg, tid);
            __syncthreads();
            ++nabs;
        } else {
            nan = MU > SX_INF_BITS || MV > SX_INF_BITS;                   // a NaN in u or v (an absorption has just replaced both)        (:646)
        }
        if (ii % pp == 0) {                                               // err = || colsum Gamma(alpha, beta, u, v) - b ||              (:623-636)
            double err = __builtin_nan("");                               // (a NaN in u or v makes every column sum, and the norm, NaN)
            if (!nan) {
                for (int i = tid; i < m1; i += SX_NT) uo[i] = log(un[i]);                // the previous u, v are dead unless the NaN exit is taken
                for (int j = tid; j < m2; j += SX_NT) vo[j] = log(vn[j]);
                __syncthreads();
                double e2 = 0.0;
                for (int j = wave; j < m2; j += SX_NW) {
                    double sum = 0.0;
                    for (int i = lane; i < m1; i += 64) sum += sx_gamma(s, reg, uo, vo, i, j);
                    sum = wave_sum_d(sum);
                    const double d = sum - s.bv[j];
                    if (lane == 0) e2 += d * d;
                }
                err = sqrt(block_sum_d<SX_NW>(e2, s.red));               // (its barriers also order these reads before the next sweep's writes)
            }
            if (!INNER && errs && tid == 0) errs[ii / pp] = (float)err;
            ++nchk;
            if (err <= thr) { flags |= 1; cur ^= 1; break; }             // (:643; err changes at a check only, and every run checks at ii = 0)
        }
        if (nan) { flags |= 2; break; }                                   // the previous u, v stay current                               (:646-652)
        cur ^= 1;
    }
    return ii < itmax ? ii : itmax - 1;
}

template <bool RES>
__global__ void __launch_bounds__(SX_NT) k_sinkhorn_stab(SxCall c) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int N1 = c.N1, N2 = c.N2;
    const int m1 = __builtin_amdgcn_readfirstlane(min(max(c.n1 ? c.n1[b] : N1, 0), N1));
    const int m2 = __builtin_amdgcn_readfirstlane(min(max(c.n2 ? c.n2[b] : N2, 0), N2));
    if (sx_padding<SX_NT>(c, b, m1, m2, tid)) return;
    const SxS s = sx_views(c, smem, RES, b, m1, m2);
    const int mm = m1 * m2;
    float *T = c.T + (size_t)b * N1 * N2;
    float *errs = c.errs ? c.errs + (size_t)b * c.nerr : nullptr;
    const double reg = c.reg, thr = c.stop_thr;

    for (int i = tid; i < m1; i += SX_NT) {
        s.av[i] = c.a ? (double)c.a[(size_t)b * N1 + i] : sx_uniform(m1);
        s.al[i] = c.wu ? c.wu[(size_t)b * N1 + i] : 0.0;
    }
    for (int j = tid; j < m2; j += SX_NT) {
        s.bv[j] = c.b ? (double)c.b[(size_t)b * N2 + j] : sx_uniform(m2);
        s.be[j] = c.wv ? c.wv[(size_t)b * N2 + j] : 0.0;
    }
    int cur = 0, flags = 0, nchk = 0, nabs = 0, niter = 0, last = 0;
    int sweeps = 0, nan_exits = 0, nan_iter = 0;
    double lsum = 0.0;
    const double *u = s.u0, *v = s.v0;
    double *lu = s.u1, *lv = s.v1;
    if (c.method == 3) {
        niter = sx_stabilized<false>(s, reg, c.num_iter_max, thr, c.tau, c.print_period, errs, cur, flags, nchk, nabs);
        sweeps = niter + 1; last = nabs;
        u = cur ? s.u1 : s.u0; v = cur ? s.v1 : s.v0; lu = cur ? s.u0 : s.u1; lv = cur ? s.v0 : s.v1;
        __syncthreads();
        for (int i = tid; i < m1; i += SX_NT) lu[i] = log(u[i]);
        for (int j = tid; j < m2; j += SX_NT) lv[j] = log(v[j]);
        __syncthreads();
        for (int t = tid; t < mm; t += SX_NT) {                           // the plan: get_Gamma(alpha, beta, u, v)                       (sinkhorn.py:677, :685)
            const int i = t / m2, j = t - i * m2;
            const double tv = sx_gamma(s, reg, lu, lv, i, j);
            lsum += (double)s.M[(size_t)i * N2 + j] * tv;
            T[(size_t)i * N2 + j] = (float)tv;
        }
    } else {
        const int itmax = max(35, c.num_iter_max);                        // (:716-717)
        double err = 1.0;
        int ncap = 0, oflags = 0, ii = 0;
        for (; ii < itmax; ++ii) {
            const double regi = (c.eps0 - reg) * exp(-(double)ii) + reg;  // (:731-732)
            int ifl = 0, ichk = 0;
            const int in = sx_stabilized<true>(s, regi, c.num_inner, thr, c.tau, 20, nullptr, cur, ifl, ichk, nabs);
            sweeps += in + 1;
            if ((ifl & 3) == 0) ++ncap;
            if (ifl & 2) { ++nan_exits; nan_iter = in; oflags |= 2; }
            u = cur ? s.u1 : s.u0; v = cur ? s.v1 : s.v0; lu = cur ? s.u0 : s.u1; lv = cur ? s.v0 : s.v1;
            __syncthreads();
            for (int i = tid; i < m1; i += SX_NT) lu[i] = log(u[i]);
            for (int j = tid; j < m2; j += SX_NT) lv[j] = log(v[j]);
            __syncthreads();
            if (ii % c.print_period == 0) {                               // err = ||colsum G - b||^2 + ||rowsum G - a||^2 of the inner solve's plan   (:756-765)
                double e2 = 0.0;
                for (int j = wave; j < m2; j += SX_NW) {
                    double sum = 0.0;
                    for (int i = lane; i < m1; i += 64) sum += sx_gamma(s, regi, lu, lv, i, j);
                    sum = wave_sum_d(sum);
                    const double d = sum - s.bv[j];
                    if (lane == 0) e2 += d * d;
                }
                const double nc = sqrt(block_sum_d<SX_NW>(e2, s.red));
                e2 = 0.0;
                for (int i = wave; i < m1; i += SX_NW) {
                    double sum = 0.0;
                    for (int j = lane; j < m2; j += 64) sum += sx_gamma(s, regi, lu, lv, i, j);
                    sum = wave_sum_d(sum);
                    const double d = sum - s.av[i];
                    if (lane == 0) e2 += d * d;
                }
                const double nr = sqrt(block_sum_d<SX_NW>(e2, s.red));
                err = nc * nc + nr * nr;
                if (errs && tid == 0) errs[ii / c.print_period] = (float)err;
                ++nchk;
            }
            const bool leave = err <= thr && ii > 35;                     // (:772)
            if (leave || ii == itmax - 1) {                               // G of the last inner solve is the result
                for (int t = tid; t < mm; t += SX_NT) {
                    const int i = t / m2, j = t - i * m2;
                    const double tv = sx_gamma(s, regi, lu, lv, i, j);
                    lsum += (double)s.M[(size_t)i * N2 + j] * tv;
                    T[(size_t)i * N2 + j] = (float)tv;
                }
                if (c.log_u) for (int i = tid; i < m1; i += SX_NT) c.log_u[(size_t)b * N1 + i] = (float)(s.al[i] / regi + lu[i]);
                if (c.log_v) for (int j = tid; j < m2; j += SX_NT) c.log_v[(size_t)b * N2 + j] = (float)(s.be[j] / regi + lv[j]);
            }
            __syncthreads();
            for (int i = tid; i < m1; i += SX_NT) s.al[i] = s.al[i] + regi * lu[i];       // the inner solve's log["alpha"], log["beta"]   (:667-668, :753-754)
            for (int j = tid; j < m2; j += SX_NT) s.be[j] = s.be[j] + regi * lv[j];
            if (leave) { oflags |= 1; break; }
        }
        niter = ii < itmax ? ii : itmax - 1;
        flags = oflags; last = ncap;
    }
    if (c.method == 3) {                                                  // logu, logv, alpha + reg log u, beta + reg log v               (:662-668)
        if (c.log_u) for (int i = tid; i < m1; i += SX_NT) c.log_u[(size_t)b * N1 + i] = (float)(s.al[i] / reg + lu[i]);
        if (c.log_v) for (int j = tid; j < m2; j += SX_NT) c.log_v[(size_t)b * N2 + j] = (float)(s.be[j] / reg + lv[j]);
        if (c.alpha) for (int i = tid; i < m1; i += SX_NT) c.alpha[(size_t)b * N1 + i] = s.al[i] + reg * lu[i];
        if (c.beta) for (int j = tid; j < m2; j += SX_NT) c.beta[(size_t)b * N2 + j] = s.be[j] + reg * lv[j];
    } else {                                                              // (each thread reads back the entries it has just folded)
        if (c.alpha) for (int i = tid; i < m1; i += SX_NT) c.alpha[(size_t)b * N1 + i] = s.al[i];
        if (c.beta) for (int j = tid; j < m2; j += SX_NT) c.beta[(size_t)b * N2 + j] = s.be[j];
    }
    const double total = block_sum_d<SX_NW>(lsum, s.red);
    if (tid == 0) {
        if (c.loss) c.loss[b] = (float)total;
        if (c.info) { int *info = c.info + b * 4; info[0] = niter; info[1] = flags; info[2] = nchk; info[3] = last; }
        if (c.extra) { int *x = c.extra + b * 4; x[0] = sweeps; x[1] = nabs; x[2] = nan_exits; x[3] = nan_iter; }
    }
}

// arg-max over the wavefront of (key, index): the largest key, the lowest index among equal keys; every lane gets the result
__device__ __forceinline__ void sx_wave_argmax(sx_u64 &k, int &idx) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const sx_u64 k2 = __shfl_xor(k, o, 64);
        const int i2 = __shfl_xor(idx, o, 64);
        const bool take = k2 > k || (k2 == k && i2 < idx);
        k = take ? k2 : k; idx = take ? i2 : idx;
    }
}

template <bool RES>
__global__ void __launch_bounds__(64) k_greenkhorn(SxCall c) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int b = blockIdx.x, lane = threadIdx.x;
    const int N1 = c.N1, N2 = c.N2;
    const int m1 = __builtin_amdgcn_readfirstlane(min(max(c.n1 ? c.n1[b] : N1, 0), N1));
    const int m2 = __builtin_amdgcn_readfirstlane(min(max(c.n2 ? c.n2[b] : N2, 0), N2));
    if (sx_padding<64>(c, b, m1, m2, lane)) return;
    const SxS s = sx_views(c, smem, RES, b, m1, m2);
    const int P = s.P, mm = m1 * m2;
    double *K = s.K, *av = s.av, *bv = s.bv, *u = s.u0, *v = s.v0, *viol = s.u1, *viol2 = s.v1;
    float *T = c.T + (size_t)b * N1 * N2;
    const double reg = c.reg, thr = c.stop_thr;

    for (int t = lane; t < mm; t += 64) {
        const int i = t / m2, j = t - i * m2;
        K[i * P + j] = exp(-(double)s.M[(size_t)i * N2 + j] / reg);
    }
    for (int i = lane; i < m1; i += 64) {
        av[i] = c.a ? (double)c.a[(size_t)b * N1 + i] : sx_uniform(m1);
        u[i] = c.wu ? exp(c.wu[(size_t)b * N1 + i]) : sx_uniform(m1);
    }
    for (int j = lane; j < m2; j += 64) {
        bv[j] = c.b ? (double)c.b[(size_t)b * N2 + j] : sx_uniform(m2);
        v[j] = c.wv ? exp(c.wv[(size_t)b * N2 + j]) : sx_uniform(m2);
    }
    __syncthreads();
    for (int i = lane; i < m1; i += 64) {                                 // viol = rowsum(u K v) - a, lane <-> row (odd pitch: conflict-free)   (sinkhorn.py:481-484)
        double sum = 0.0;
        for (int j = 0; j < m2; ++j) sum += (u[i] * K[i * P + j]) * v[j];
        viol[i] = sum - av[i];
    }
    for (int j = lane; j < m2; j += 64) {                                 // viol_2 = colsum(u K v) - b, lane <-> column
        double sum = 0.0;
        for (int i = 0; i < m1; ++i) sum += (u[i] * K[i * P + j]) * v[j];
        viol2[j] = sum - bv[j];
    }
    __syncthreads();

    int ii = 0, flags = 0;
    for (; ii < c.num_iter_max; ++ii) {
        sx_u64 k1 = 0, k2 = 0;                                            // bit patterns of |x|: integer order is numeric order, a NaN sorts highest as in torch.argmax
        int i1 = 0, i2 = 0;
        for (int i = lane; i < m1; i += 64) { const sx_u64 k = sx_absbits(viol[i]); if (i == lane || k > k1) { k1 = k; i1 = i; } }
        for (int j = lane; j < m2; j += 64) { const sx_u64 k = sx_absbits(viol2[j]); if (j == lane || k > k2) { k2 = k; i2 = j; } }
        if (lane >= m1) i1 = 0x7fffffff;
        if (lane >= m2) i2 = 0x7fffffff;
        sx_wave_argmax(k1, i1);
        sx_wave_argmax(k2, i2);
        i1 = __builtin_amdgcn_readfirstlane(i1); i2 = __builtin_amdgcn_readfirstlane(i2);
        const double mv1 = __longlong_as_double((long long)k1), mv2 = __longlong_as_double((long long)k2);
        if (mv1 > mv2) {                                                  // the row i1                                                   (:498-505)
            const double *Kr = K + i1 * P;
            double dot = 0.0;
            for (int j = lane; j < m2; j += 64) dot += Kr[j] * v[j];
            dot = wave_sum_d(dot);
            const double old_u = u[i1], new_u = av[i1] / dot, du = new_u - old_u;
            double dot2 = 0.0;
            for (int j = lane; j < m2; j += 64) {
                const double kj = Kr[j], vj = v[j];
                dot2 += (new_u * kj) * vj;
                viol2[j] = viol2[j] + (kj * du) * vj;
            }
            dot2 = wave_sum_d(dot2);
            __syncthreads();                                              // (every lane has read u[i1])
            if (lane == 0) { viol[i1] = dot2 - av[i1]; u[i1] = new_u; }
        } else {                                                          // the column i2                                                (:507-514)
            const double *Kc = K + i2;
            double dot = 0.0;
            for (int i = lane; i < m1; i += 64) dot += Kc[i * P] * u[i];
            dot = wave_sum_d(dot);
            const double old_v = v[i2], new_v = bv[i2] / dot, dv = -old_v + new_v;
            for (int i = lane; i < m1; i += 64) viol[i] = viol[i] + (dv * Kc[i * P]) * u[i];
            __syncthreads();
            if (lane == 0) { viol2[i2] = new_v * dot - bv[i2]; v[i2] = new_v; }
        }
        __syncthreads();
        if (mv1 <= thr && mv2 <= thr) { flags = 1; break; }               // maximum(m_viol_1, m_viol_2) <= stopThr; a NaN maximum compares false   (:516)
    }
    double lsum = 0.0;
    for (int t = lane; t < mm; t += 64) {                                 // G = (u K) v at exit
        const int i = t / m2, j = t - i * m2;
        const double tv = (u[i] * K[i * P + j]) * v[j];
        lsum += (double)s.M[(size_t)i * N2 + j] * tv;
        T[(size_t)i * N2 + j] = (float)tv;
    }
    if (c.log_u) for (int i = lane; i < m1; i += 64) c.log_u[(size_t)b * N1 + i] = (float)log(u[i]);
    if (c.log_v) for (int j = lane; j < m2; j += 64) c.log_v[(size_t)b * N2 + j] = (float)log(v[j]);
    if (c.alpha) for (int i = lane; i < m1; i += 64) c.alpha[(size_t)b * N1 + i] = 0.0;
    if (c.beta) for (int j = lane; j < m2; j += 64) c.beta[(size_t)b * N2 + j] = 0.0;
    lsum = wave_sum_d(lsum);
    if (lane == 0) {
        const int niter = ii < c.num_iter_max ? ii : c.num_iter_max - 1;
        if (c.loss) c.loss[b] = (float)lsum;
        if (c.info) { int *info = c.info + b * 4; info[0] = niter; info[1] = flags; info[2] = 0; info[3] = 0; }
        if (c.extra) { int *x = c.extra + b * 4; x[0] = niter + 1; x[1] = 0; x[2] = 0; x[3] = 0; }
    }
}

}  // namespace

extern "C" {

int conan_sinkhorn_ext_lds_resident(int n1, int n2) {
    if (n1 <= 0 || n2 <= 0) return 0;
    return sx_vec_bytes(n1, n2) + sx_mat_bytes(n1, n2) <= LDS_LIMIT ? 1 : 0;
}

long long conan_sinkhorn_ext_workspace_bytes(int B, int N1, int N2) {
    if (B <= 0 || N1 <= 0 || N2 <= 0 || sx_vec_bytes(N1, N2) > LDS_LIMIT || sx_mat_bytes(N1, N2) / 8 >= (size_t)1 << 31) return 0;
    if (conan_sinkhorn_ext_lds_resident(N1, N2)) return 256;              // nothing is streamed; a non-empty buffer keeps the pointer valid
    return (long long)((size_t)B * al256(sx_mat_bytes(N1, N2)));
}

int conan_sinkhorn_ext_nerr(int method, int num_iter_max, int print_period) {
    if (method == 2) return 0;
    if ((method != 3 && method != 4) || num_iter_max <= 0 || print_period <= 0) return -1;
    const long long it = method == 4 ? (num_iter_max < 35 ? 35 : num_iter_max) : num_iter_max;
    return (int)((it + print_period - 1) / print_period);
}

int conan_sinkhorn_ext_fwd(const float *M, const float *a, const float *b, const double *warm_u, const double *warm_v, const int *n1, const int *n2, int B,
                           int N1, int N2, long long m_batch_stride, double reg, int method, int num_iter_max, double stop_thr, double tau,
                           int print_period, double epsilon0, int num_inner_iter_max, float *T, float *loss, float *log_u, float *log_v, double *alpha,
                           double *beta, int *info, float *errs, int *extra, void *workspace, void *stream) {
    if (!M || !T || !workspace || B <= 0 || N1 <= 0 || N2 <= 0 || num_iter_max <= 0 || m_batch_stride < 0) return CONAN_E_BADARG;
    if (!(reg > 0.0) || !(reg < __builtin_inf()) || method < 2 || method > 4 || stop_thr != stop_thr) return CONAN_E_BADARG;
    if (method != 2 && (!(tau > 0.0) || print_period <= 0)) return CONAN_E_BADARG;
    if (method == 4 && (num_inner_iter_max <= 0 || !(epsilon0 > -__builtin_inf() && epsilon0 < __builtin_inf()))) return CONAN_E_BADARG;
    if (conan_sinkhorn_ext_workspace_bytes(B, N1, N2) == 0) return CONAN_E_UNSUPPORTED;
    SxCall c{};
    c.M = M; c.a = a; c.b = b; c.wu = warm_u; c.wv = warm_v; c.n1 = n1; c.n2 = n2;
    c.N1 = N1; c.N2 = N2; c.method = method; c.num_iter_max = num_iter_max; c.print_period = print_period; c.num_inner = num_inner_iter_max;
    c.nerr = conan_sinkhorn_ext_nerr(method, num_iter_max, print_period);
    c.m_stride = m_batch_stride;
    c.reg = reg; c.stop_thr = stop_thr; c.tau = tau; c.eps0 = epsilon0;
    c.T = T; c.loss = loss; c.log_u = log_u; c.log_v = log_v; c.alpha = alpha; c.beta = beta; c.errs = c.nerr > 0 ? errs : nullptr;
    c.info = info; c.extra = extra;
    c.ws = static_cast<double *>(workspace); c.ws_stride = al256(sx_mat_bytes(N1, N2)) / 8;
    const hipStream_t s = as_stream(stream);
    const bool res = conan_sinkhorn_ext_lds_resident(N1, N2) != 0;
    const size_t lds = sx_vec_bytes(N1, N2) + (res ? sx_mat_bytes(N1, N2) : 0);
    if (method == 2) {
        if (res) launch_lds(k_greenkhorn<true>, B, 64, lds, s, c);
        else launch_lds(k_greenkhorn<false>, B, 64, lds, s, c);
    } else {
        if (res) launch_lds(k_sinkhorn_stab<true>, B, SX_NT, lds, s, c);
        else launch_lds(k_sinkhorn_stab<false>, B, SX_NT, lds, s, c);
    }
    CONAN_LAUNCH_CHECK();
    return CONAN_OK;
}

}  // extern "C"
