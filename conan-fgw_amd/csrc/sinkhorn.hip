// Entropic optimal transport on its own for gfx950: the reference's sinkhorn_log (sinkhorn.py:318-450, method 0) and sinkhorn_knopp (:207-315,
// method 1) for B problems per launch, one workgroup of SK_NW wavefronts per problem (conan_sinkhorn_fwd; DESIGN.md 3.3, "Sinkhorn on its own").
//
// Sizes.  Problem b is n1[b] x n2[b] (device-side, nullable: N1 x N2) inside an [N1, N2] container.  Rectangular problems are native: every loop
// runs over the problem's own rows and columns, the matrix has the problem's own pitch P = n2[b] | 1, and nothing outside the block is read.
// Outputs outside the block are written as zeros.
//
// Arithmetic.  fp32 in and out, fp64 in between.  Both methods iterate on a fixed fp64 matrix K [n1, P] and two fp64 vectors:
//     column pass   s_j = sum_i K_ij u_i,  v_j = b_j / s_j          one wavefront per column, lane <-> row    (stride P, odd: conflict-free)
//     row pass      r_i = sum_j K_ij v_j,  u_i = a_i / r_i          one wavefront per row,    lane <-> column (stride 1)
//     check (ii % 10 == 0)   err = || v o (K^T u) - b ||_2, stop when err < stop_thr
// Knopp: K = exp(M / -reg), u = 1 / n1, v = 1 / n2 or exp(warm start), u_i = 1 / sum_j ((1 / a_i) K_ij) v_j as the reference forms it, so that
// its numerical-errors exit (a zero K^T u, a NaN or Inf in u or v: previous u, v restored, flag bit 1) is decided on the same fp64 values.
// sinkhorn_log: the same scaling iteration on K_ij = exp(Mr_ij - ref_j), Mr = -M / reg, ref_j = max_i Mr_ij, u = 1 or exp(warm start).  The
// reference's potentials are log u_i and log v_j - ref_j.  A column whose exp(Mr) underflows fp64 altogether (M / reg > 745) is therefore
// exact: its largest entry is 1.  An entry of K below fp64's range is dropped; with every sum of a pass kept inside [1e-100, 1e100] such an
// entry of the plan is below 1e-120.  A sum outside that range (or not finite) sends the problem to the exact log-domain iteration
// (flag bit 2), restarted from the warm start: max-shifted log-sum-exp with fp64 exp / log, -inf potentials for zero weights.
// A zero entry of a (of b) gives u_i = 0 (v_j = 0), an exactly zero row (column), and takes part in the first column pass with u_i = 1 as in
// the reference (unlike the FGW solve's embedding, fgw_coupling.h, which keeps massless nodes out of it).
// Every sum is fp64 in a fixed order (per lane in index order, then the xor butterfly over the 64 lanes, then the wavefronts in order): no
// atomics, nothing shared between workgroups, every loop bounded by num_iter_max.  The order depends on n1[b], n2[b] alone, so a problem gives
// the same bits alone, in any batch, at any position and in any container, LDS-resident or streamed.
//
// Storage.  K lives in LDS when the CONTAINER fits ((16 + 3 N1 + 4 N2 + N1 (N2 | 1)) * 8 bytes <= 160 KiB: conan_sinkhorn_lds_resident), else every problem of the
// launch streams it from its slice of the workspace (L2-resident at these sizes); the vectors are always in LDS.
#include "fgw_common.h"
namespace {
constexpr int SK_NW = 4, SK_NT = 64 * SK_NW;

struct SkCall {
    const float *M, *a, *b, *wu, *wv;
    const int *n1, *n2;
    int N1, N2, method, num_iter_max, nerr;
    long long m_stride;
    double reg, stop_thr;          // widened on the host: the scalar unit has no fp64 conversions
    float *T, *loss, *log_u, *log_v, *errs;
    int *info;
    double *ws;
    size_t ws_stride;              // doubles per problem
};

inline size_t sk_vec_bytes(int N1, int N2) { return (size_t)(16 + 3 * (size_t)N1 + 4 * (size_t)N2) * 8; }
inline size_t sk_mat_bytes(int N1, int N2) { return (size_t)N1 * (size_t)(N2 | 1) * 8; }

__device__ __forceinline__ bool sk_bad(double x) { return !(x > 1e-100 && x < 1e100); }
__device__ __forceinline__ bool sk_naninf(double x) { return !(fabs(x) < __builtin_inf()); }

template <bool RES>
__global__ void __launch_bounds__(SK_NT) k_sinkhorn(SkCall c) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int N1 = c.N1, N2 = c.N2;
    const int m1 = __builtin_amdgcn_readfirstlane(min(max(c.n1 ? c.n1[b] : N1, 0), N1));
    const int m2 = __builtin_amdgcn_readfirstlane(min(max(c.n2 ? c.n2[b] : N2, 0), N2));
    const int P = m2 | 1, mm = m1 * m2;
    double *red = reinterpret_cast<double *>(smem);
    int *flag = reinterpret_cast<int *>(red + 14);                        // slots 0 / 1: one per iteration parity, slot 2: the set-up; never cleared: a set flag ends the loop
    double *av = red + 16, *u0 = av + N1, *u1 = u0 + N1, *bv = u1 + N1, *v0 = bv + N2, *v1 = v0 + N2, *ref = v1 + N2;
    double *K;
    if constexpr (RES) K = ref + N2;
    else K = c.ws + (size_t)b * c.ws_stride;
    const float *M = c.M + (size_t)b * (size_t)c.m_stride;
    float *T = c.T + (size_t)b * N1 * N2;
    float *errs = c.errs ? c.errs + (size_t)b * c.nerr : nullptr;
    const double reg = c.reg;
    const bool knopp = c.method == 1;

    // padding of the container and the untouched checks
    for (int t = tid; t < N1 * N2; t += SK_NT) {
        const int i = t / N2, j = t - i * N2;
        if (i >= m1 || j >= m2) T[t] = 0.f;
    }
    if (c.log_u) for (int i = m1 + tid; i < N1; i += SK_NT) c.log_u[(size_t)b * N1 + i] = 0.f;
    if (c.log_v) for (int j = m2 + tid; j < N2; j += SK_NT) c.log_v[(size_t)b * N2 + j] = 0.f;
    if (errs) for (int t = tid; t < c.nerr; t += SK_NT) errs[t] = __builtin_nanf("");
    if (m1 == 0 || m2 == 0) {                                             // (workgroup-uniform)
        if (c.info && tid < 4) c.info[b * 4 + tid] = 0;
        if (c.loss && tid == 0) c.loss[b] = 0.f;
        return;
    }

    for (int i = tid; i < m1; i += SK_NT) av[i] = c.a ? (double)c.a[(size_t)b * N1 + i] : 1.0 / (double)m1;
    for (int j = tid; j < m2; j += SK_NT) bv[j] = c.b ? (double)c.b[(size_t)b * N2 + j] : 1.0 / (double)m2;
    if (tid < 3) flag[tid] = 0;
    if (knopp) {
        for (int t = tid; t < mm; t += SK_NT) {
            const int i = t / m2, j = t - i * m2;
            K[i * P + j] = exp((double)M[(size_t)i * N2 + j] / -reg);
        }
        for (int i = tid; i < m1; i += SK_NT) u0[i] = c.wu ? exp((double)c.wu[(size_t)b * N1 + i]) : 1.0 / (double)m1;
        for (int j = tid; j < m2; j += SK_NT) { v0[j] = c.wv ? exp((double)c.wv[(size_t)b * N2 + j]) : 1.0 / (double)m2; ref[j] = 0.0; }
        __syncthreads();
    } else {
        for (int t = tid; t < mm; t += SK_NT) {
            const int i = t / m2, j = t - i * m2;
            K[i * P + j] = -(double)M[(size_t)i * N2 + j] / reg;
        }
        __syncthreads();
        for (int j = wave; j < m2; j += SK_NW) {                          // ref_j = max_i Mr_ij
            double mx = -__builtin_inf();
            for (int i = lane; i < m1; i += 64) mx = fmax(mx, K[i * P + j]);
            mx = wave_max_d(mx);
            if (lane == 0) { ref[j] = mx; if (sk_naninf(mx)) flag[2] = 1; }
        }
        for (int i = tid; i < m1; i += SK_NT) {
            const double u = c.wu ? exp((double)c.wu[(size_t)b * N1 + i]) : 1.0;
            if (sk_bad(u)) flag[2] = 1;
            u0[i] = u;
        }
        for (int j = tid; j < m2; j += SK_NT) v0[j] = 0.0;
        __syncthreads();
        if (flag[2] == 0)
            for (int t = tid; t < mm; t += SK_NT) {
                const int i = t / m2, j = t - i * m2;
                K[i * P + j] = exp(K[i * P + j] - ref[j]);
            }
        __syncthreads();
    }

    int ii = 0, flags = 0, nchk = 0, cur = 0;
    bool exact = !knopp && flag[2] != 0;
    if (!exact) {
        for (; ii < c.num_iter_max; ++ii) {
            const double *uo = cur ? u1 : u0, *vo = cur ? v1 : v0;
            double *un = cur ? u0 : u1, *vn = cur ? v0 : v1;
            int *fl = flag + (ii & 1);
            (void)vo;
            for (int j = wave; j < m2; j += SK_NW) {                      // v = b / (K^T u)                              (sinkhorn.py:258-259, :415)
                double s = 0.0;
                for (int i = lane; i < m1; i += 64) s += K[i * P + j] * uo[i];
                s = wave_sum_d(s);
                if (lane == 0) {
                    const double vj = bv[j] / s;
                    vn[j] = vj;
                    if (knopp ? (s == 0.0 || sk_naninf(vj)) : sk_bad(s)) *fl = 1;
                }
            }
            __syncthreads();
            for (int i = wave; i < m1; i += SK_NW) {                      // u = 1 / ((K / a) v)  resp.  a / (K v)          (sinkhorn.py:260, :416)
                double s = 0.0, ui;
                if (knopp) {
                    const double ia = 1.0 / av[i];
                    for (int j = lane; j < m2; j += 64) s += (ia * K[i * P + j]) * vn[j];
                    s = wave_sum_d(s);
                    ui = 1.0 / s;
                    if (lane == 0 && sk_naninf(ui)) *fl = 1;
                } else {
                    for (int j = lane; j < m2; j += 64) s += K[i * P + j] * vn[j];
                    s = wave_sum_d(s);
                    ui = av[i] / s;
                    if (lane == 0 && sk_bad(s)) *fl = 1;
                }
                if (lane == 0) un[i] = ui;
            }
            __syncthreads();
            if (*fl != 0) {                                               // (workgroup-uniform: read after the barrier that published it)
                if (knopp) flags |= 2;                                    // numerical errors: the previous u, v stay current (sinkhorn.py:262-274)
                else exact = true;
                break;
            }
            cur ^= 1;
            if (ii % 10 == 0) {                                           // violation of the column marginal                  (sinkhorn.py:275-288, :418-433)
                double e2 = 0.0;
                for (int j = wave; j < m2; j += SK_NW) {
                    double s = 0.0;
                    for (int i = lane; i < m1; i += 64) s += K[i * P + j] * un[i];
                    s = wave_sum_d(s);
                    const double d = vn[j] * s - bv[j];
                    if (lane == 0) e2 += d * d;
                }
                const double err = sqrt(block_sum_d<SK_NW>(e2, red));
                if (errs && tid == 0) errs[ii / 10] = (float)err;
                ++nchk;
                if (err < c.stop_thr) { flags |= 1; break; }
            }
        }
    }
    const double *u = cur ? u1 : u0, *v = cur ? v1 : v0;
    double lsum = 0.0;
    if (!exact) {
        for (int t = tid; t < mm; t += SK_NT) {                           // T = diag(u) K diag(v); loss = sum M o T
            const int i = t / m2, j = t - i * m2;
            const double tv = u[i] * K[i * P + j] * v[j];
            lsum += (double)M[(size_t)i * N2 + j] * tv;
            T[(size_t)i * N2 + j] = (float)tv;
        }
        if (c.log_u) for (int i = tid; i < m1; i += SK_NT) c.log_u[(size_t)b * N1 + i] = (float)log(u[i]);
        if (c.log_v) for (int j = tid; j < m2; j += SK_NT) c.log_v[(size_t)b * N2 + j] = (float)(log(v[j]) - ref[j]);
    } else {
        // ---- the exact log-domain iteration (sinkhorn.py:393-433) from the start: K holds Mr, u0 / v0 the potentials
        flags = 4; nchk = 0;
        double *lu = u0, *lv = v0;
        __syncthreads();
        if (errs) for (int t = tid; t < c.nerr; t += SK_NT) errs[t] = __builtin_nanf("");
        for (int t = tid; t < mm; t += SK_NT) {
            const int i = t / m2, j = t - i * m2;
            K[i * P + j] = -(double)M[(size_t)i * N2 + j] / reg;
        }
        for (int i = tid; i < m1; i += SK_NT) lu[i] = c.wu ? (double)c.wu[(size_t)b * N1 + i] : 0.0;
        for (int j = tid; j < m2; j += SK_NT) lv[j] = c.wv ? (double)c.wv[(size_t)b * N2 + j] : 0.0;
        __syncthreads();
        for (ii = 0; ii < c.num_iter_max; ++ii) {
            for (int j = wave; j < m2; j += SK_NW) {                      // v_j = log b_j - logsumexp_i(Mr_ij + u_i)
                double mx = -__builtin_inf();
                for (int i = lane; i < m1; i += 64) mx = fmax(mx, K[i * P + j] + lu[i]);
                mx = wave_max_d(mx);
                double s = 0.0;
                if (!sk_naninf(mx))
                    for (int i = lane; i < m1; i += 64) s += exp(K[i * P + j] + lu[i] - mx);
                s = wave_sum_d(s);
                if (lane == 0) lv[j] = log(bv[j]) - (sk_naninf(mx) ? mx : log(s) + mx);
            }
            __syncthreads();
            for (int i = wave; i < m1; i += SK_NW) {                      // u_i = log a_i - logsumexp_j(Mr_ij + v_j)
                double mx = -__builtin_inf();
                for (int j = lane; j < m2; j += 64) mx = fmax(mx, K[i * P + j] + lv[j]);
                mx = wave_max_d(mx);
                double s = 0.0;
                if (!sk_naninf(mx))
                    for (int j = lane; j < m2; j += 64) s += exp(K[i * P + j] + lv[j] - mx);
                s = wave_sum_d(s);
                if (lane == 0) lu[i] = log(av[i]) - (sk_naninf(mx) ? mx : log(s) + mx);
            }
            __syncthreads();
            if (ii % 10 == 0) {
                double e2 = 0.0;
                for (int j = wave; j < m2; j += SK_NW) {
                    double s = 0.0;
                    for (int i = lane; i < m1; i += 64) s += exp(K[i * P + j] + lu[i] + lv[j]);
                    s = wave_sum_d(s);
                    const double d = s - bv[j];
                    if (lane == 0) e2 += d * d;
                }
                const double err = sqrt(block_sum_d<SK_NW>(e2, red));     // (its barriers also order these reads before the next updates)
                if (errs && tid == 0) errs[ii / 10] = (float)err;
                ++nchk;
                if (err < c.stop_thr) { flags |= 1; break; }
            }
        }
        for (int t = tid; t < mm; t += SK_NT) {
            const int i = t / m2, j = t - i * m2;
            const double tv = exp(K[i * P + j] + lu[i] + lv[j]);
            lsum += (double)M[(size_t)i * N2 + j] * tv;
            T[(size_t)i * N2 + j] = (float)tv;
        }
        if (c.log_u) for (int i = tid; i < m1; i += SK_NT) c.log_u[(size_t)b * N1 + i] = (float)lu[i];
        if (c.log_v) for (int j = tid; j < m2; j += SK_NT) c.log_v[(size_t)b * N2 + j] = (float)lv[j];
    }
    const double total = block_sum_d<SK_NW>(lsum, red);
    if (tid == 0) {
        if (c.loss) c.loss[b] = (float)total;
        if (c.info) {
            int *info = c.info + b * 4;
            info[0] = ii < c.num_iter_max ? ii : c.num_iter_max - 1;     // the reference's log["niter"]: the loop index at exit
            info[1] = flags; info[2] = nchk; info[3] = 0;
        }
    }
}

}  // namespace

extern "C" {

int conan_sinkhorn_lds_resident(int n1, int n2) {
    if (n1 <= 0 || n2 <= 0) return 0;
    return sk_vec_bytes(n1, n2) + sk_mat_bytes(n1, n2) <= LDS_LIMIT ? 1 : 0;
}

long long conan_sinkhorn_workspace_bytes(int B, int N1, int N2) {
    if (B <= 0 || N1 <= 0 || N2 <= 0 || sk_vec_bytes(N1, N2) > LDS_LIMIT || sk_mat_bytes(N1, N2) / 8 >= (size_t)1 << 31) return 0;
    if (conan_sinkhorn_lds_resident(N1, N2)) return 256;                  // nothing is streamed; a non-empty buffer keeps the pointer valid
    return (long long)((size_t)B * al256(sk_mat_bytes(N1, N2)));
}

int conan_sinkhorn_fwd(const float *M, const float *a, const float *b, const float *warm_u, const float *warm_v, const int *n1, const int *n2, int B,
                       int N1, int N2, long long m_batch_stride, float reg, int method, int num_iter_max, float stop_thr, float *T, float *loss,
                       float *log_u, float *log_v, int *info, float *errs, void *workspace, void *stream) {
    if (!M || !T || !workspace || B <= 0 || N1 <= 0 || N2 <= 0 || num_iter_max <= 0 || m_batch_stride < 0) return CONAN_E_BADARG;
    if (!(reg > 0.f) || !(reg < __builtin_inff()) || method < 0 || method > 1) return CONAN_E_BADARG;
    if (conan_sinkhorn_workspace_bytes(B, N1, N2) == 0) return CONAN_E_UNSUPPORTED;
    SkCall c{};
    c.M = M; c.a = a; c.b = b; c.wu = warm_u; c.wv = warm_v; c.n1 = n1; c.n2 = n2;
    c.N1 = N1; c.N2 = N2; c.method = method; c.num_iter_max = num_iter_max; c.nerr = (num_iter_max + 9) / 10;
    c.m_stride = m_batch_stride;
    c.reg = (double)reg; c.stop_thr = (double)stop_thr;
    c.T = T; c.loss = loss; c.log_u = log_u; c.log_v = log_v; c.errs = errs; c.info = info;
    c.ws = static_cast<double *>(workspace); c.ws_stride = al256(sk_mat_bytes(N1, N2)) / 8;
    const hipStream_t s = as_stream(stream);
    if (conan_sinkhorn_lds_resident(N1, N2)) launch_lds(k_sinkhorn<true>, B, SK_NT, sk_vec_bytes(N1, N2) + sk_mat_bytes(N1, N2), s, c);
    else launch_lds(k_sinkhorn<false>, B, SK_NT, sk_vec_bytes(N1, N2), s, c);
    CONAN_LAUNCH_CHECK();
    return CONAN_OK;
}

}  // extern "C"
