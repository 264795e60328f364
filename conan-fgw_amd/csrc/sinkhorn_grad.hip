// The reference's gradient through the unrolled Sinkhorn sweeps for gfx950: the backward of conan_sinkhorn_fwd (sinkhorn.hip, methods 0
// sinkhorn_log and 1 sinkhorn_knopp) to M, a, b and warmstart[0], B problems per launch, one workgroup of SK_NW wavefronts per problem
// (conan_sinkhorn_bwd; DESIGN.md 3.3, "The unrolled gradient").
//
// Both methods are the iteration  g^t = log b - LSE_i(Mr + f^(t-1)),  f^t = log a - LSE_j(Mr + g^t),  t = 1..S,  T = exp(Mr + f^S + g^S),
// Mr = -M / reg, f = log u, g = log v.  In the scaling form every term below is u_i K_ij v_j, which does not depend on the gauge: the column
// shift ref_j of sinkhorn_log and Knopp's 1 / n start drop out.  With the cotangents gl (of the loss sum(M o T)) and dT (of the plan):
//     Tb = gl M + dT,   fb_i = sum_j Tb_ij T_ij,   gb_j = sum_i Tb_ij T_ij
//     for t = S..1:   z = fb o u^t / a;   la += fb;   gb -= v^t o (K^T z);       fb = 0          (row pass t)
//                     w = gb o v^t / b;   lb += gb;   fb -= u^(t-1) o (K w);     gb = 0          (column pass t)
//     dMr = K o (-sum_t [z^t (x) v^t + u^(t-1) (x) w^t]) + Tb o T
//     dM = gl T - dMr / reg,   da = la / a,   db = lb / b,   d warmstart[0] = fb after the loop;   warmstart[1] gets none (the first column
// pass overwrites v).  A zero entry of a (of b) contributes nothing (z_i = 0, w_j = 0) and its own weight gradient is written as 0.
// S = info[0] + 1 - ((info[1] >> 1) & 1), clamped to [0, num_iter_max] (sinkhorn_log: to [1, num_iter_max], it always executes a sweep): the
// sweeps the forward executed; Knopp's numerical-errors exit restored the previous u, v.  The stop decision carries no gradient.
//
// Three steps.  (1) The S sweeps are recomputed from the fp32 inputs, without checks, on the path info names (scaling form, or the exact
// log-domain form when flag bit 2 is set: max-shifted log-sum-exp, fp64 exp / log, entries exp(Mr + f + g) per pass), and u^t, v^t (f^t, g^t)
// stored in the problem's slice of the workspace.  (2) The reverse sweeps, two matrix-vector passes each like the forward's, store z^t, w^t.
// (3) dMr is ONE product over the stored histories, P [n1, 2S] = [z^1.. | u^0..], Q [n2, 2S] = [v^1.. | w^1..]: 64 x 64 output tiles, a 4 x 4
// block of fp64 accumulators per thread, the histories staged through LDS BW_TC sweeps at a time.  No second N1 x N2 matrix, no read-modify-write
// of a matrix per sweep.  (The exact path sums its 2 S entries exp(Mr + f + g) per element straight from the histories: it is rare.)
//
// Conventions of k_sinkhorn: per-problem sizes inside the [N1, N2] container, pitch P = n2 | 1, fp32 in and out, fp64 in between, every sum in
// a fixed order that depends on n1[b], n2[b] and S alone (per lane in index order, the xor butterfly, then t ascending), no atomics, nothing
// shared between workgroups, zeros outside a problem's block.  K is LDS-resident when (16 + 5 N1 + 5 N2 + N1 (N2 | 1)) * 8 + 16384 bytes <= 160
// KiB (conan_sinkhorn_bwd_lds_resident), else streamed from the workspace; the arithmetic is the same code on both paths: the same bits.
// Workspace per problem: ((2 num_iter_max + 1) (N1 + N2) + [streamed] N1 (N2 | 1)) * 8 bytes, rounded up to 256.
#include "fgw_common.h"
namespace {
constexpr int SK_NW = 4, SK_NT = 64 * SK_NW;
constexpr int BW_TC = 8;                                   // sweeps per staged chunk of the final product (2 BW_TC columns of P and Q)
constexpr size_t BW_STAGE_BYTES = (size_t)2 * (2 * BW_TC) * 64 * 8;

struct SkBwdCall {
    const float *M, *a, *b, *wu, *wv;
    const int *n1, *n2, *info;
    const float *gl, *gT;
    float *dM, *da, *db, *dwu;
    int N1, N2, method, num_iter_max;
    long long m_stride;
    double reg;                    // widened on the host: the scalar unit has no fp64 conversions
    double *ws;
    size_t ws_stride;              // doubles per problem
};

inline size_t skb_vec_bytes(int N1, int N2) { return (size_t)(16 + 5 * (size_t)N1 + 5 * (size_t)N2) * 8 + BW_STAGE_BYTES; }
inline size_t skb_mat_bytes(int N1, int N2) { return (size_t)N1 * (size_t)(N2 | 1) * 8; }
inline size_t skb_hist_doubles(int N1, int N2, int it) { return (size_t)(2 * (size_t)it + 1) * ((size_t)N1 + (size_t)N2); }

__device__ __forceinline__ bool skb_naninf(double x) { return !(fabs(x) < __builtin_inf()); }

template <bool RES>
__global__ void __launch_bounds__(SK_NT) k_sinkhorn_bwd(SkBwdCall c) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int N1 = c.N1, N2 = c.N2;
    const int m1 = __builtin_amdgcn_readfirstlane(min(max(c.n1 ? c.n1[b] : N1, 0), N1));
    const int m2 = __builtin_amdgcn_readfirstlane(min(max(c.n2 ? c.n2[b] : N2, 0), N2));
    const int P = m2 | 1, mm = m1 * m2;
    const int itmax = c.num_iter_max;
    double *red = reinterpret_cast<double *>(smem);
    double *av = red + 16, *fb = av + N1, *la = fb + N1, *zc = la + N1, *uc = zc + N1;              // uc / vc: u^(t-1), v^t of the recomputation (f, g on the exact path)
    double *bv = uc + N1, *gb = bv + N2, *lb = gb + N2, *wc = lb + N2, *vc = wc + N2;
    double *Pst = vc + N2, *Qst = Pst + 2 * BW_TC * 64;
    double *hU = c.ws + (size_t)b * c.ws_stride;                         // u^0 .. u^itmax [itmax + 1][N1]
    double *hZ = hU + (size_t)(itmax + 1) * N1;                           // z^1 .. z^itmax [itmax][N1]
    double *hV = hZ + (size_t)itmax * N1;                                 // v^0 .. v^itmax [itmax + 1][N2]
    double *hW = hV + (size_t)(itmax + 1) * N2;                           // w^1 .. w^itmax [itmax][N2]
    double *K;
    if constexpr (RES) K = Qst + 2 * BW_TC * 64;
    else K = hW + (size_t)itmax * N2;
    const float *M = c.M + (size_t)b * (size_t)c.m_stride;
    const float *gT = c.gT ? c.gT + (size_t)b * N1 * N2 : nullptr;
    float *dM = c.dM + (size_t)b * N1 * N2;
    const double reg = c.reg;
    const bool knopp = c.method == 1;

    // padding of the container
    for (int t = tid; t < N1 * N2; t += SK_NT) {
        const int i = t / N2, j = t - i * N2;
        if (i >= m1 || j >= m2) dM[t] = 0.f;
    }
    if (c.da) for (int i = m1 + tid; i < N1; i += SK_NT) c.da[(size_t)b * N1 + i] = 0.f;
    if (c.dwu) for (int i = m1 + tid; i < N1; i += SK_NT) c.dwu[(size_t)b * N1 + i] = 0.f;
    if (c.db) for (int j = m2 + tid; j < N2; j += SK_NT) c.db[(size_t)b * N2 + j] = 0.f;
    if (m1 == 0 || m2 == 0) return;                                        // (workgroup-uniform)

    const int flags = __builtin_amdgcn_readfirstlane(c.info[b * 4 + 1]);
    const bool exact = !knopp && (flags & 4) != 0;
    int S = min(max(c.info[b * 4], 0), itmax) + 1 - ((flags >> 1) & 1);   // (niter clamped first: no overflow in the sum)
    S = __builtin_amdgcn_readfirstlane(min(max(S, knopp ? 0 : 1), itmax)); // a corrupt info can neither leave the workspace nor lengthen a loop
    const double gl = c.gl ? (double)c.gl[b] : 0.0;

    for (int i = tid; i < m1; i += SK_NT) { av[i] = c.a ? (double)c.a[(size_t)b * N1 + i] : 1.0 / (double)m1; fb[i] = 0.0; la[i] = 0.0; }
    for (int j = tid; j < m2; j += SK_NT) { bv[j] = c.b ? (double)c.b[(size_t)b * N2 + j] : 1.0 / (double)m2; gb[j] = 0.0; lb[j] = 0.0; }

    // ---- step 1: K and the S sweeps again, histories to the workspace ------------------------------------------------------------------
    if (knopp) {
        for (int t = tid; t < mm; t += SK_NT) {
            const int i = t / m2, j = t - i * m2;
            K[i * P + j] = exp((double)M[(size_t)i * N2 + j] / -reg);
        }
        for (int i = tid; i < m1; i += SK_NT) uc[i] = c.wu ? exp((double)c.wu[(size_t)b * N1 + i]) : 1.0 / (double)m1;
        for (int j = tid; j < m2; j += SK_NT) vc[j] = c.wv ? exp((double)c.wv[(size_t)b * N2 + j]) : 1.0 / (double)m2;
    } else {
        for (int t = tid; t < mm; t += SK_NT) {
            const int i = t / m2, j = t - i * m2;
            K[i * P + j] = -(double)M[(size_t)i * N2 + j] / reg;
        }
        if (!exact) {
            __syncthreads();
            for (int j = wave; j < m2; j += SK_NW) {                      // ref_j = max_i Mr_ij (kept in wc until K is formed)
                double mx = -__builtin_inf();
                for (int i = lane; i < m1; i += 64) mx = fmax(mx, K[i * P + j]);
                mx = wave_max_d(mx);
                if (lane == 0) wc[j] = mx;
            }
            __syncthreads();
            for (int t = tid; t < mm; t += SK_NT) {
                const int i = t / m2, j = t - i * m2;
                K[i * P + j] = exp(K[i * P + j] - wc[j]);
            }
            for (int i = tid; i < m1; i += SK_NT) uc[i] = c.wu ? exp((double)c.wu[(size_t)b * N1 + i]) : 1.0;
        } else {
            for (int i = tid; i < m1; i += SK_NT) uc[i] = c.wu ? (double)c.wu[(size_t)b * N1 + i] : 0.0;
        }
        for (int j = tid; j < m2; j += SK_NT) vc[j] = 0.0;               // (never read: sinkhorn_log executes at least one sweep)
    }
    __syncthreads();
    for (int i = tid; i < m1; i += SK_NT) hU[i] = uc[i];
    for (int j = tid; j < m2; j += SK_NT) hV[j] = vc[j];

    for (int t = 1; t <= S; ++t) {
        double *ut = hU + (size_t)t * N1, *vt = hV + (size_t)t * N2;
        if (!exact) {
            for (int j = wave; j < m2; j += SK_NW) {                      // v = b / (K^T u)
                double s = 0.0;
                for (int i = lane; i < m1; i += 64) s += K[i * P + j] * uc[i];
                s = wave_sum_d(s);
                if (lane == 0) { const double vj = bv[j] / s; vc[j] = vj; vt[j] = vj; }
            }
            __syncthreads();
            for (int i = wave; i < m1; i += SK_NW) {                      // u = 1 / ((K / a) v)  resp.  a / (K v), as the forward forms them
                double s = 0.0, ui;
                if (knopp) {
                    const double ia = 1.0 / av[i];
                    for (int j = lane; j < m2; j += 64) s += (ia * K[i * P + j]) * vc[j];
                    s = wave_sum_d(s);
                    ui = 1.0 / s;
                } else {
                    for (int j = lane; j < m2; j += 64) s += K[i * P + j] * vc[j];
                    s = wave_sum_d(s);
                    ui = av[i] / s;
                }
                if (av[i] == 0.0) ui = 0.0;
                if (lane == 0) { uc[i] = ui; ut[i] = ui; }
            }
            __syncthreads();
        } else {
            for (int j = wave; j < m2; j += SK_NW) {                      // g_j = log b_j - logsumexp_i(Mr_ij + f_i)
                double mx = -__builtin_inf();
                for (int i = lane; i < m1; i += 64) mx = fmax(mx, K[i * P + j] + uc[i]);
                mx = wave_max_d(mx);
                double s = 0.0;
                if (!skb_naninf(mx))
                    for (int i = lane; i < m1; i += 64) s += exp(K[i * P + j] + uc[i] - mx);
                s = wave_sum_d(s);
                if (lane == 0) { const double gj = log(bv[j]) - (skb_naninf(mx) ? mx : log(s) + mx); vc[j] = gj; vt[j] = gj; }
            }
            __syncthreads();
            for (int i = wave; i < m1; i += SK_NW) {                      // f_i = log a_i - logsumexp_j(Mr_ij + g_j)
                double mx = -__builtin_inf();
                for (int j = lane; j < m2; j += 64) mx = fmax(mx, K[i * P + j] + vc[j]);
                mx = wave_max_d(mx);
                double s = 0.0;
                if (!skb_naninf(mx))
                    for (int j = lane; j < m2; j += 64) s += exp(K[i * P + j] + vc[j] - mx);
                s = wave_sum_d(s);
                if (lane == 0) { const double fi = log(av[i]) - (skb_naninf(mx) ? mx : log(s) + mx); uc[i] = fi; ut[i] = fi; }
            }
            __syncthreads();
        }
    }
    __syncthreads();                                                       // (S = 0: publishes uc, vc and the histories)

    // ---- step 2: the cotangents of the final potentials, then the reverse sweeps --------------------------------------------------------
    // plan entry at the potentials in uc, vc
    auto plan = [&](int i, int j) -> double { return exact ? exp(K[i * P + j] + uc[i] + vc[j]) : uc[i] * K[i * P + j] * vc[j]; };
    auto tbar = [&](int i, int j) -> double { return gl * (double)M[(size_t)i * N2 + j] + (gT ? (double)gT[(size_t)i * N2 + j] : 0.0); };
    for (int i = wave; i < m1; i += SK_NW) {                              // fb_i = sum_j Tb_ij T_ij
        double s = 0.0;
        for (int j = lane; j < m2; j += 64) s += tbar(i, j) * plan(i, j);
        s = wave_sum_d(s);
        if (lane == 0) fb[i] = s;
    }
    for (int j = wave; j < m2; j += SK_NW) {                              // gb_j = sum_i Tb_ij T_ij
        double s = 0.0;
        for (int i = lane; i < m1; i += 64) s += tbar(i, j) * plan(i, j);
        s = wave_sum_d(s);
        if (lane == 0) gb[j] = s;
    }
    __syncthreads();

    for (int t = S; t >= 1; --t) {
        const double *ut = hU + (size_t)t * N1, *up = ut - N1, *vt = hV + (size_t)t * N2;
        double *zt = hZ + (size_t)(t - 1) * N1, *wt = hW + (size_t)(t - 1) * N2;
        // row pass t
        for (int i = tid; i < m1; i += SK_NT) {
            const double f = fb[i], ai = av[i];
            const double z = ai != 0.0 ? (exact ? f / ai : f * ut[i] / ai) : 0.0;
            la[i] += f; fb[i] = 0.0; zc[i] = z; zt[i] = z;
            if (exact) uc[i] = ut[i];
        }
        if (exact) for (int j = tid; j < m2; j += SK_NT) vc[j] = vt[j];
        __syncthreads();
        for (int j = wave; j < m2; j += SK_NW) {                          // gb -= v^t o (K^T z)
            double s = 0.0;
            if (exact) for (int i = lane; i < m1; i += 64) s += zc[i] * exp(K[i * P + j] + uc[i] + vc[j]);
            else for (int i = lane; i < m1; i += 64) s += K[i * P + j] * zc[i];
            s = wave_sum_d(s);
            if (lane == 0) gb[j] -= exact ? s : vt[j] * s;
        }
        __syncthreads();
        // column pass t
        for (int j = tid; j < m2; j += SK_NT) {
            const double g = gb[j], bj = bv[j];
            const double w = bj != 0.0 ? (exact ? g / bj : g * vt[j] / bj) : 0.0;
            lb[j] += g; gb[j] = 0.0; wc[j] = w; wt[j] = w;
        }
        if (exact) for (int i = tid; i < m1; i += SK_NT) uc[i] = up[i];
        __syncthreads();
        for (int i = wave; i < m1; i += SK_NW) {                          // fb -= u^(t-1) o (K w)
            double s = 0.0;
            if (exact) for (int j = lane; j < m2; j += 64) s += wc[j] * exp(K[i * P + j] + uc[i] + vc[j]);
            else for (int j = lane; j < m2; j += 64) s += K[i * P + j] * wc[j];
            s = wave_sum_d(s);
            if (lane == 0) fb[i] -= exact ? s : up[i] * s;
        }
        __syncthreads();
    }

    for (int i = tid; i < m1; i += SK_NT) {
        if (c.da) c.da[(size_t)b * N1 + i] = av[i] != 0.0 ? (float)(la[i] / av[i]) : 0.f;
        if (c.dwu) c.dwu[(size_t)b * N1 + i] = (float)fb[i];
    }
    if (c.db) for (int j = tid; j < m2; j += SK_NT) c.db[(size_t)b * N2 + j] = bv[j] != 0.0 ? (float)(lb[j] / bv[j]) : 0.f;

    // ---- step 3: dMr from the histories, dM out -------------------------------------------------------------------------------------------
    const double *uS = hU + (size_t)S * N1, *vS = hV + (size_t)S * N2;
    if (exact) {
        for (int e = tid; e < mm; e += SK_NT) {
            const int i = e / m2, j = e - i * m2;
            const double mr = K[i * P + j];
            double acc = 0.0;
            for (int t = 1; t <= S; ++t) {
                const double g = hV[(size_t)t * N2 + j];
                acc += hZ[(size_t)(t - 1) * N1 + i] * exp(mr + hU[(size_t)t * N1 + i] + g);
                acc += hW[(size_t)(t - 1) * N2 + j] * exp(mr + hU[(size_t)(t - 1) * N1 + i] + g);
            }
            const double tv = exp(mr + uS[i] + vS[j]);
            const double dmr = -acc + tbar(i, j) * tv;
            dM[(size_t)i * N2 + j] = (float)(gl * tv - dmr / reg);
        }
        return;
    }
    const int ty = tid >> 4, tx = tid & 15;
    for (int i0 = 0; i0 < m1; i0 += 64)
        for (int j0 = 0; j0 < m2; j0 += 64) {
            double acc[4][4];
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int q = 0; q < 4; ++q) acc[r][q] = 0.0;
            for (int t0 = 0; t0 < S; t0 += BW_TC) {
                const int nt = min(BW_TC, S - t0);
                __syncthreads();
                for (int e = tid; e < 2 * nt * 64; e += SK_NT) {          // columns k < nt: z^(t0+k+1), v^(t0+k+1); k >= nt: u^(t0+k-nt), w^(t0+k-nt+1)
                    const int k = e >> 6, r = e & 63, i = i0 + r, j = j0 + r;
                    const size_t tp = k < nt ? (size_t)(t0 + k) : (size_t)(t0 + k - nt);
                    const double *ph = k < nt ? hZ : hU, *qh = k < nt ? hV + N2 : hW;
                    Pst[e] = i < m1 ? ph[tp * N1 + i] : 0.0;
                    Qst[e] = j < m2 ? qh[tp * N2 + j] : 0.0;
                }
                __syncthreads();
                for (int k = 0; k < 2 * nt; ++k) {
                    double p[4], q[4];
#pragma unroll
                    for (int r = 0; r < 4; ++r) { p[r] = Pst[k * 64 + ty + 16 * r]; q[r] = Qst[k * 64 + tx + 16 * r]; }
#pragma unroll
                    for (int r = 0; r < 4; ++r)
#pragma unroll
                        for (int s = 0; s < 4; ++s) acc[r][s] = fma(p[r], q[s], acc[r][s]);
                }
            }
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    const int i = i0 + ty + 16 * r, j = j0 + tx + 16 * s;
                    if (i < m1 && j < m2) {
                        const double kij = K[i * P + j];
                        const double tv = uS[i] * kij * vS[j];
                        const double dmr = -(kij * acc[r][s]) + tbar(i, j) * tv;
                        dM[(size_t)i * N2 + j] = (float)(gl * tv - dmr / reg);
                    }
                }
        }
}

}  // namespace

extern "C" {

int conan_sinkhorn_bwd_lds_resident(int n1, int n2) {
    if (n1 <= 0 || n2 <= 0) return 0;
    return skb_vec_bytes(n1, n2) + skb_mat_bytes(n1, n2) <= LDS_LIMIT ? 1 : 0;
}

long long conan_sinkhorn_bwd_workspace_bytes(int B, int N1, int N2, int num_iter_max) {
    if (B <= 0 || N1 <= 0 || N2 <= 0 || num_iter_max <= 0 || skb_vec_bytes(N1, N2) > LDS_LIMIT || skb_mat_bytes(N1, N2) / 8 >= (size_t)1 << 31) return 0;
    const size_t per = skb_hist_doubles(N1, N2, num_iter_max) * 8 + (conan_sinkhorn_bwd_lds_resident(N1, N2) ? 0 : skb_mat_bytes(N1, N2));
    return (long long)((size_t)B * al256(per));
}

int conan_sinkhorn_bwd(const float *M, const float *a, const float *b, const float *warm_u, const float *warm_v, const int *n1, const int *n2, int B,
                       int N1, int N2, long long m_batch_stride, float reg, int method, int num_iter_max, const int *info, const float *gloss,
                       const float *gT, float *dM, float *da, float *db, float *dwu, void *workspace, void *stream) {
    if (!M || !info || !dM || !workspace || B <= 0 || N1 <= 0 || N2 <= 0 || num_iter_max <= 0 || m_batch_stride < 0) return CONAN_E_BADARG;
    if (!gloss && !gT) return CONAN_E_BADARG;
    if (!(reg > 0.f) || !(reg < __builtin_inff()) || method < 0 || method > 1) return CONAN_E_BADARG;
    if (conan_sinkhorn_bwd_workspace_bytes(B, N1, N2, num_iter_max) == 0) return CONAN_E_UNSUPPORTED;
    const bool res = conan_sinkhorn_bwd_lds_resident(N1, N2) != 0;
    SkBwdCall c{};
    c.M = M; c.a = a; c.b = b; c.wu = warm_u; c.wv = warm_v; c.n1 = n1; c.n2 = n2; c.info = info;
    c.gl = gloss; c.gT = gT; c.dM = dM; c.da = da; c.db = db; c.dwu = dwu;
    c.N1 = N1; c.N2 = N2; c.method = method; c.num_iter_max = num_iter_max;
    c.m_stride = m_batch_stride;
    c.reg = (double)reg;
    c.ws = static_cast<double *>(workspace);
    c.ws_stride = al256(skb_hist_doubles(N1, N2, num_iter_max) * 8 + (res ? 0 : skb_mat_bytes(N1, N2))) / 8;
    const hipStream_t s = as_stream(stream);
    if (res) launch_lds(k_sinkhorn_bwd<true>, B, SK_NT, skb_vec_bytes(N1, N2) + skb_mat_bytes(N1, N2), s, c);
    else launch_lds(k_sinkhorn_bwd<false>, B, SK_NT, skb_vec_bytes(N1, N2), s, c);
    CONAN_LAUNCH_CHECK();
    return CONAN_OK;
}

}  // extern "C"
