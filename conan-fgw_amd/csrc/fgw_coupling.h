#pragma once
#include "fgw_common.h"
namespace {
// The general coupling solve, one per workgroup (SECOND: one per flagged coupling of the workgroup's 64): k_fgw_coupling (fgw.hip) and k_fgw_coupling_pair (fgw_pair.hip)
// are this function.  Parameters and arguments are k_fgw_coupling's (described there), then PAIR and `pr` (by reference: by value measured slower); with PAIR, Yw, active, Ypart, Cpart, only and adj.rowptr are null.
template <int MODE, bool KL, int NW, bool SECOND, bool PPA, bool ASYM, bool PAIR>
__device__ __forceinline__ void fgw_coupling_solve(
    const float *__restrict__ Ys, const float *__restrict__ Cs, const float *__restrict__ ps, const float *__restrict__ pb, FgwDims D, conan_fgw_params prm,
    int outer, int y_zero, const double *__restrict__ Cw, const double *__restrict__ Yw, const int *__restrict__ active, float *__restrict__ Tw,
    int *__restrict__ info, char *__restrict__ scratch, fgw_part_t *__restrict__ Ypart, fgw_part_t *__restrict__ Cpart, const int *__restrict__ only,
    FgwAdj adj, const FgwPair &pr) {
    constexpr bool LDS_MODE = MODE == 2, MR_LDS = MODE >= 1;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int NT = 64 * NW;
    [[maybe_unused]] int sym_auto = 0;                                  // ASYM: symmetric=None (decided per coupling solve)
    if constexpr (ASYM) { sym_auto = y_zero >> 1; y_zero &= 1; }
    auto solve = [&](const int cid) {
    const int b = cid / D.K, s = cid % D.K;
    if constexpr (!PAIR) { if (!fgw_active(active, D.B, b, outer)) return; }
    const int N = D.N, P = D.P, d = D.d;
    const int NN = N * N, NP = N * P;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    FGW_PROF_DECL;

    // ---- carve
    double *vec = reinterpret_cast<double *>(smem);          // [(6 + 2 NW)*N + 16] : u, v, loga, logb, r1/y2, r2/z2, red, pm[NW][N], psm[NW][N]
    double *u = vec, *v = vec + N, *loga = vec + 2 * N, *logb = vec + 3 * N, *ra = vec + 4 * N, *rb = vec + 5 * N;
    double *red = vec + 6 * N;
    double *pm = red + 16, *psm = pm + NW * N;                // per-wavefront partial (max, sum) of the log-sum-exp loops
    // LDS_MODE: all four matrices in LDS.  Otherwise only the Sinkhorn cost Mr (read 2x per Sinkhorn iteration, once by
    // rows and once by columns) stays in LDS when it fits (mr_lds); A, base and T live in an L2-resident global scratch.
    char *gs = scratch + (size_t)cid * coupling_scratch_stride(NP);     // 16-byte aligned per coupling
    char *ls = smem + (size_t)((6 + 2 * NW) * N + 16) * 8;
    double *Mr = MR_LDS ? reinterpret_cast<double *>(ls) : reinterpret_cast<double *>(gs);
    double *Al = LDS_MODE ? Mr + NP : reinterpret_cast<double *>(gs) + NP;
    double *base = Al + NP;
    float *Tl = reinterpret_cast<float *>(base + NP);

    const float *Z = Ys + ((size_t)b * D.K + s) * N * d;        // features of input graph s      [N,d]
    // structure of input graph s [N,N]; with the ragged structure (FgwAdj) this kernel is only the exact pass behind k_fgw_coupling_big, and a
    // flagged coupling expands its graph into its own slice of the dense scratch first
    const float *C2 = adj.rowptr ? adj_dense_slice<NT>(adj, cid, N, tid) : Cs + ((size_t)b * D.K + s) * NN;
    const double *C1 = Cw + (size_t)b * NN;                     // current barycenter structure   [N,N]
    const double *Y = Yw + (size_t)b * N * d;                   // current barycenter features    [N,d]
    float *Tg = Tw + ((size_t)b * D.K + s) * NN;
    const double alpha = (double)prm.alpha, eps = (double)prm.epsilon;

    // ---- marginals: p (barycenter), q = ps[s]; uniform when not given (barycenter.py:50-51, schnet_no_sum.py:264-279)
    for (int i = tid; i < N; i += NT) {
        const double pi = pb ? (double)pb[(size_t)b * N + i] : 1.0 / (double)N;
        const double qi = ps ? (double)ps[((size_t)b * D.K + s) * N + i] : 1.0 / (double)N;
        loga[i] = log(pi); logb[i] = log(qi);
        u[i] = pi; v[i] = qi;                                  // temporarily hold p, q
    }
    __syncthreads();
    // ---- T0: warm start from the previous outer iteration, else outer(p, q)      (bregman.py:98-101)
    for (int t = tid; t < NN; t += NT) {
        const int i = t / N, j = t - i * N;
        const float t0 = (outer > 0 && prm.warmstart) ? Tg[t] : (float)(u[i] * v[j]);
        Tl[i * P + j] = t0;
        Mr[i * P + j] = (double)t0;     // the coupling also lives (fp64) where the Sinkhorn state K will: the products read it from there
    }
    // ---- init_matrix (utils.py:39-43): constC[i][j] = sum_k C1[i,k]^2 p_k + sum_k q_k C2[j,k]^2 ; squared feature norms
    double *y2a = Al, *z2a = Al + N;                            // Al is not live yet
    {   // 8 lanes per index, strided partial sums combined by xor-shuffles (fixed order): one thread per index walked N + d
        // dependent L2 round trips
        constexpr int LPI = 8;
        for (int i0 = 0; i0 < N; i0 += NT / LPI) {
            const int i = i0 + tid / LPI, sub = tid % LPI;
            double r1 = 0.0, r2 = 0.0, y2 = 0.0, z2 = 0.0;
            if (i < N) {
                for (int k = sub; k < N; k += LPI) {
                    const double c1 = C1[i * N + k], c2 = (double)C2[i * N + k];
                    r1 += (KL ? c1 * log(c1 + 1e-15) - c1 : c1 * c1) * u[k];
                    r2 += v[k] * (KL ? c2 : c2 * c2);
                }
                for (int c = sub; c < d; c += LPI) {
                    const double yy = Y[i * d + c], zz = (double)Z[i * d + c];
                    y2 += yy * yy; z2 += zz * zz;
                }
            }
#pragma unroll
            for (int o = 1; o < LPI; o <<= 1) {
                r1 += __shfl_xor(r1, o, 64); r2 += __shfl_xor(r2, o, 64); y2 += __shfl_xor(y2, o, 64); z2 += __shfl_xor(z2, o, 64);
            }
            if (i < N && sub == 0) { ra[i] = r1; rb[i] = r2; y2a[i] = y2; z2a[i] = z2; }
        }
    }
    // ASYM: c'_i = sum_k f1(C1[k,i]) p_k and r'_j = sum_k q_k f2(C2[k,j]) (init_matrix of the transposes) in pm[0:N] / pm[N:2N] (not live
    // before the Sinkhorn loop), and the symmetry test of symmetric=None, |x_ik - x_ki| <= 1e-10 + 1e-5 |x_ki| (torch.allclose)
    [[maybe_unused]] bool asym = false;
    if constexpr (ASYM) {
        int nonsym = 0;
        constexpr int LPI = 8;
        for (int i0 = 0; i0 < N; i0 += NT / LPI) {
            const int i = i0 + tid / LPI, sub = tid % LPI;
            double r1 = 0.0, r2 = 0.0;
            if (i < N)
                for (int k = sub; k < N; k += LPI) {
                    const double c1t = C1[k * N + i], c2t = (double)C2[k * N + i];
                    r1 += (KL ? c1t * log(c1t + 1e-15) - c1t : c1t * c1t) * u[k];
                    r2 += v[k] * (KL ? c2t : c2t * c2t);
                    if (sym_auto) {
                        const double c1 = C1[i * N + k], c2 = (double)C2[i * N + k];
                        nonsym |= !(fabs(c1 - c1t) <= 1e-10 + 1e-5 * fabs(c1t)) || !(fabs(c2 - c2t) <= 1e-10 + 1e-5 * fabs(c2t));
                    }
                }
#pragma unroll
            for (int o = 1; o < LPI; o <<= 1) { r1 += __shfl_xor(r1, o, 64); r2 += __shfl_xor(r2, o, 64); }
            if (i < N && sub == 0) { pm[i] = r1; pm[N + i] = r2; }
        }
        if constexpr (CONAN_FGW_ASYM_C1T && MODE >= 1) {      // C1^T into the slice's first N x P doubles (Mr's place in mode 0: unused in 1 / 2)
            double *c1t = reinterpret_cast<double *>(gs);
            for (int t = tid; t < NN; t += NT) { const int i = t / N, k = t - i * N; c1t[t] = C1[k * N + i]; }
        }
        asym = !sym_auto || __syncthreads_or(nonsym) != 0;              // (workgroup-uniform)
    }
    __syncthreads();
    FGW_PROF(0);      // staging: T0, per-index vectors
    // ---- base = alpha*2*constC + (1-alpha)*M,  M = clamp(|y_i|^2 + |z_j|^2 - 2 y_i.z_j, 0)   (utils.py:154-171, bregman.py:124-125)
    // dot(Y_i, Z_j) on fp64 MFMA straight from global memory (L2-resident), then the elementwise assembly
    if (!y_zero)
        mm_f64_glb<NW, true>(N, N, d, Y, d, Z, d, [&](int i, int j, double v) { base[i * P + j] = v; });
    __syncthreads();
    FGW_PROF(1);      // dot(Y, Z)
    for (int t = tid; t < NN; t += NT) {
        const int i = t / N, j = t - i * N;
        double m = -2.0 * (y_zero ? 0.0 : base[i * P + j]);    // utils.py:159-161
        m += y2a[i]; m += z2a[j];
        m = m > 0.0 ? m : 0.0;                                  // :163
        if constexpr (PAIR) m = (double)pr.M[(size_t)b * NN + t];     // the caller's cost, as given (not clamped: bregman.py:125)
        if constexpr (ASYM) {
            if (asym) { base[i * P + j] = alpha * (ra[i] + pm[i] + rb[j] + pm[N + j]) + (1.0 - alpha) * m; continue; }
        }
        base[i * P + j] = 2.0 * alpha * (ra[i] + rb[j]) + (1.0 - alpha) * m;
    }
    __syncthreads();
    int zero_mass = 0;
    for (int i = tid; i < N; i += NT) { ra[i] = exp(loga[i]); rb[i] = exp(logb[i]); zero_mass |= (loga[i] < -1.0e300 || logb[i] < -1.0e300) ? 1 : 0; }      // p_i, q_j for the scaling form (r1 / r2 are consumed)
    double *pa = ra, *qb = rb;
    // nodes without mass (fgw.py embeds n != N problems with such nodes): the scaling form's first half-step would count them (g = 1 on every
    // row), so such couplings take the log-domain path, whose potentials start at -inf there
    const bool massless = __syncthreads_or(zero_mass) != 0;
    FGW_PROF(2);      // base

    // ---- projected gradient loop (bregman.py:119-157)
    int cpt = 0, sk_total = 0;
    [[maybe_unused]] int ppa_zero = 0;                                  // PPA: a row / column of the kernel matrix vanished (flags bit 2)
    double err = 1.0;
    while (err > (double)prm.inner_tol && cpt < prm.max_iter) {
        // A = C1 @ T ; G = A @ (2 C2)^T on fp64 MFMA ; tens = base - 2*alpha*G ; Mr = -tens/eps
        // (utils.py:48-64, bregman.py:124-125, sinkhorn.py:388)
        // W operand: the coupling as the Sinkhorn state left it in Mr's storage (LDS in modes 1 / 2; the fp32-rounded T in an
        // fp64 container) instead of the fp32 copy in the global scratch: half of this product's memory accesses
        mm_f64_glb<NW, false>(N, N, N, C1, N, Mr, P, [&](int i, int j, double v) { Al[i * P + j] = v; });
        __syncthreads();
        FGW_PROF(3);  // A = C1 @ T
        auto form_mr = [&]() {
            if constexpr (ASYM) {
                if (asym) {      // G1 = A h2(C2)^T into Mr; B = C1^T T into Al (A is consumed); tens = base - alpha' (G1 + B h2(C2))
                    if constexpr (KL)
                        mm_f64<NW>(N, N, N, [&](int i, int k) { return Al[i * P + k]; }, [&](int k, int j) { return log((double)C2[j * N + k] + 1e-15); },
                               [&](int i, int j, double g) { Mr[i * P + j] = g; });
                    else
                        mm_f64_glb<NW, true>(N, N, N, Al, P, C2, N, [&](int i, int j, double g) { Mr[i * P + j] = g; });
                    __syncthreads();
                    // T from its fp32 copy (the fp64 one in Mr's storage is gone): the same values
                    if constexpr (CONAN_FGW_ASYM_C1T && MODE >= 1)
                        mm_f64_glb<NW, false>(N, N, N, reinterpret_cast<const double *>(gs), N, Tl, P, [&](int i, int j, double v) { Al[i * P + j] = v; });
                    else
                        mm_f64<NW>(N, N, N, [&](int i, int k) { return C1[k * N + i]; }, [&](int k, int j) { return (double)Tl[k * P + j]; },
                                   [&](int i, int j, double v) { Al[i * P + j] = v; });
                    __syncthreads();
                    if constexpr (KL)
                        mm_f64<NW>(N, N, N, [&](int i, int k) { return Al[i * P + k]; }, [&](int k, int j) { return log((double)C2[k * N + j] + 1e-15); },
                               [&](int i, int j, double g) { Mr[i * P + j] = -(base[i * P + j] - alpha * (Mr[i * P + j] + g)) / eps; });
                    else      // hC2 = 2 C2
                        mm_f64_glb<NW, false>(N, N, N, Al, P, C2, N,
                                              [&](int i, int j, double g) { Mr[i * P + j] = -(base[i * P + j] - 2.0 * alpha * (Mr[i * P + j] + g)) / eps; });
                    return;
                }
            }
            if constexpr (KL)
                mm_f64<NW>(N, N, N, [&](int i, int k) { return Al[i * P + k]; }, [&](int k, int j) { return log((double)C2[j * N + k] + 1e-15); },
                       [&](int i, int j, double g) { Mr[i * P + j] = -(base[i * P + j] - 2.0 * alpha * g) / eps; });
            else
                mm_f64_glb<NW, true>(N, N, N, Al, P, C2, N,
                                     [&](int i, int j, double g) { Mr[i * P + j] = -(base[i * P + j] - 4.0 * alpha * g) / eps; });      // hC2 = 2 C2
        };
        form_mr();
        __syncthreads();
        FGW_PROF(4);  // G, Mr
        // ---- Sinkhorn in its matrix-scaling form, in place on Mr (see fgw_small.hip): K = exp(Mr - Mr_jj) with the first column
        // step folded in, then alternating passes   K <- K diag(f), row sums -> g = a / rowsum   (lane <-> row)   and
        // K <- diag(g) K, column sums -> f = b / colsum   (lane <-> column): one multiply-add per entry and half-iteration instead
        // of two exp.  After a row-scaled pass K is exp(Mr + u + v) of the reference iteration (sinkhorn.py:415-416), its column
        // sums are the marginal check (:418-433) and feed the next v update.  A sum outside [1e-150, 1e150] (or not finite) sends
        // the call to the exact log-domain path below.  u[] holds the row factors g, v[] the column factors f.
        int ii = 0;
        bool exact = false;
        auto bad = [](double x) { return !(x > 1e-150 && x < 1e150); };
        static_assert(NW < 15, "red[15] is the range flag: block_sum_d<NW> must not reach it");
        double *bad_flag = red + 15;                                      // set by whoever sees a sum out of range; read after the next barrier
        for (int j = tid; j < N; j += NT) v[j] = Mr[j * P + j];          // column references (the diagonal), before K overwrites them
        if (tid == 0) *bad_flag = massless ? 1.0 : 0.0;
        __syncthreads();
        for (int j = lane; j < N; j += 64) {                              // K = exp(Mr - ref_j), partial column sums
            const double ref = v[j];
            double cs = 0.0;
            for (int i = wave; i < N; i += NW) {
                double k = exp_fast(Mr[i * P + j] - ref);
                if constexpr (PPA) k *= (double)Tl[i * P + j];              // (Tl: the previous coupling until the T store below)
                Mr[i * P + j] = k; cs += k;
            }
            psm[wave * N + j] = cs;
        }
        __syncthreads();
        for (int j = tid; j < N; j += NT) {
            double cs = 0.0;
#pragma unroll
            for (int w = 0; w < NW; ++w) cs += psm[w * N + j];
            if (bad(cs)) *bad_flag = 1.0;
            v[j] = qb[j] / cs;                                            // f_j of the first v update (u = 0)
        }
        __syncthreads();
        exact = *bad_flag != 0.0;                                         // workgroup-uniform: read after the barrier that published it
        FGW_PROF(5);  // K = exp(Mr - ref), first column step
        for (; !exact && ii < prm.num_iter_max; ++ii) {
            // K <- K diag(f); row sums                                                         (sinkhorn.py:415 applied, :416 prepared)
            for (int i = lane; i < N; i += 64) {
                double rs = 0.0;
                for (int j = wave; j < N; j += NW) { const double k = Mr[i * P + j] * v[j]; Mr[i * P + j] = k; rs += k; }
                pm[wave * N + i] = rs;
            }
            __syncthreads();
            for (int i = tid; i < N; i += NT) {
                double rs = 0.0;
#pragma unroll
                for (int w = 0; w < NW; ++w) rs += pm[w * N + i];
                if (bad(rs)) *bad_flag = 1.0;
                u[i] = pa[i] / rs;
            }
            __syncthreads();
            if (*bad_flag != 0.0) { exact = true; break; }
            // K <- diag(g) K; column sums = marginals of the iterate                           (sinkhorn.py:416 applied)
            for (int j = lane; j < N; j += 64) {
                double cs = 0.0;
                for (int i = wave; i < N; i += NW) { const double k = Mr[i * P + j] * u[i]; Mr[i * P + j] = k; cs += k; }
                psm[wave * N + j] = cs;
            }
            __syncthreads();
            double e2 = 0.0;
            for (int j = tid; j < N; j += NT) {
                double cs = 0.0;
#pragma unroll
                for (int w = 0; w < NW; ++w) cs += psm[w * N + j];
                if (bad(cs)) *bad_flag = 1.0;
                const double df = cs - qb[j];
                e2 += df * df;
                v[j] = qb[j] / cs;                                        // f_j of the next v update
            }
            if (ii % 10 == 0) {                                           // marginal violation, sinkhorn.py:418-433
                const double tot = block_sum_d<NW>(e2, red);              // (its barriers publish v[] and the flag)
                if (*bad_flag != 0.0) { exact = true; break; }
                if (sqrt(tot) < (double)prm.stop_thr) { ++ii; break; }
            } else {
                __syncthreads();
                if (*bad_flag != 0.0) { exact = true; break; }
            }
        }
        if (exact) {
            // ---- exact log-domain Sinkhorn (sinkhorn.py:393-433), restarted from u = v = 0 on a re-formed Mr
            __syncthreads();
            if constexpr (ASYM) {
                if (asym) {      // Al holds B = C1^T T: A = C1 T again, T from its fp32 copy
                    mm_f64_glb<NW, false>(N, N, N, C1, N, Tl, P, [&](int i, int j, double v) { Al[i * P + j] = v; });
                    __syncthreads();
                }
            }
            form_mr();
            if constexpr (PPA) {
                __syncthreads();
                for (int t = tid; t < NN; t += NT) {
                    const int i = t / N, j = t - i * N;
                    const float tp = Tl[i * P + j];
                    Mr[i * P + j] = tp > 0.f ? Mr[i * P + j] + log((double)tp) : -__builtin_inf();
                }
            }
            // (a node without mass has log-weight -inf and its potential is -inf after its first update; it starts there, so that it never
            // enters the other side's first log-sum-exp: the rectangular problem fgw.py embeds has no such node at all)
            for (int i = tid; i < N; i += NT) { u[i] = loga[i] < -1.0e300 ? loga[i] : 0.0; v[i] = logb[i] < -1.0e300 ? logb[i] : 0.0; }     // sinkhorn.py:393-394
            __syncthreads();
            for (ii = 0; ii < prm.num_iter_max; ++ii) {
                // v_j = logb_j - logsumexp_i(Mr_ij + u_i).  lane <-> column (consecutive lanes read consecutive LDS words), the
                // wavefronts split the rows: serial (max, sum) per thread, no cross-lane fp64 reductions; the partials per column
                // are combined through LDS.
                for (int j = lane; j < N; j += 64) {
                    double mx = -1.0e300;
                    for (int i = wave; i < N; i += NW) { const double z = Mr[i * P + j] + u[i]; mx = fmax(z, mx); }
                    double sm = 0.0;
                    for (int i = wave; i < N; i += NW) sm += exp_lse(Mr[i * P + j] + u[i] - mx);      // argument <= 0: fp32 exponent unit
                    pm[wave * N + j] = mx; psm[wave * N + j] = sm;
                }
                __syncthreads();
                for (int j = tid; j < N; j += NT) {
                    double M = pm[j];
#pragma unroll
                    for (int w = 1; w < NW; ++w) M = fmax(M, pm[w * N + j]);
                    double sm = 0.0;
#pragma unroll
                    for (int w = 0; w < NW; ++w) sm += psm[w * N + j] * exp_lse(pm[w * N + j] - M);
                    if constexpr (PPA) {      // a column that is -inf throughout: massless (stays -inf), or the reference's NaN case
                        if (!(sm > 0.0)) { v[j] = logb[j] < -1.0e300 ? logb[j] : __builtin_inf(); if (logb[j] >= -1.0e300) ppa_zero = 1; continue; }
                    }
                    v[j] = logb[j] - (log_acc(sm) + M);
                }
                __syncthreads();
                // u_i = loga_i - logsumexp_j(Mr_ij + v_j): lane <-> row (odd pitch: conflict-free), wavefronts split the columns
                for (int i = lane; i < N; i += 64) {
                    double mx = -1.0e300;
                    for (int j = wave; j < N; j += NW) { const double z = Mr[i * P + j] + v[j]; mx = fmax(z, mx); }
                    double sm = 0.0;
                    for (int j = wave; j < N; j += NW) sm += exp_lse(Mr[i * P + j] + v[j] - mx);
                    pm[wave * N + i] = mx; psm[wave * N + i] = sm;
                }
                __syncthreads();
                for (int i = tid; i < N; i += NT) {
                    double M = pm[i];
#pragma unroll
                    for (int w = 1; w < NW; ++w) M = fmax(M, pm[w * N + i]);
                    double sm = 0.0;
#pragma unroll
                    for (int w = 0; w < NW; ++w) sm += psm[w * N + i] * exp_lse(pm[w * N + i] - M);
                    if constexpr (PPA) {
                        if (!(sm > 0.0)) { u[i] = loga[i] < -1.0e300 ? loga[i] : __builtin_inf(); if (loga[i] >= -1.0e300) ppa_zero = 1; continue; }
                    }
                    u[i] = loga[i] - (log_acc(sm) + M);
                }
                __syncthreads();
                if (ii % 10 == 0) {                                 // marginal violation, sinkhorn.py:418-433
                    for (int j = lane; j < N; j += 64) {
                        double sm = 0.0;
                        for (int i = wave; i < N; i += NW) sm += exp_acc(Mr[i * P + j] + u[i] + v[j]);
                        psm[wave * N + j] = sm;
                    }
                    __syncthreads();
                    double e2 = 0.0;
                    for (int j = tid; j < N; j += NT) {
                        double cs = 0.0;
#pragma unroll
                        for (int w = 0; w < NW; ++w) cs += psm[w * N + j];
                        const double df = cs - qb[j];
                        e2 += df * df;
                    }
                    const double tot = block_sum_d<NW>(e2, red);
                    if (sqrt(tot) < (double)prm.stop_thr) { ++ii; break; }
                }
            }
            for (int t = tid; t < NN; t += NT) {                    // K = exp(Mr + u + v) in place: both paths hand the same state on
                const int i = t / N, j = t - i * N;
                Mr[i * P + j] = exp_acc(Mr[i * P + j] + u[i] + v[j]);
            }
            __syncthreads();
        }
        sk_total += ii;
        FGW_PROF(6);  // Sinkhorn iterations
        // ---- T = exp(Mr + u + v) (sinkhorn.py:450); err = ||T - Tprev||_F evaluated when cpt % 10 == 0 (bregman.py:144-147)
        double e2 = 0.0;
        for (int t = tid; t < NN; t += NT) {
            const int i = t / N, j = t - i * N;
            const float tn = (float)Mr[i * P + j];                  // the scaled coupling = exp(Mr + u + v), sinkhorn.py:450
            const double df = (double)tn - (double)Tl[i * P + j];
            e2 += df * df;
            Tl[i * P + j] = tn;
            Mr[i * P + j] = (double)tn;                             // the products read T from here: the same fp32-rounded values that are returned
        }
        if (cpt % 10 == 0) {
            err = sqrt(block_sum_d<NW>(e2, red));
            if constexpr (PAIR) { if (tid == 0) pr.errs[(size_t)b * pr.nerr + cpt / 10] = (float)err; }      // log["err"] (bregman.py:149-150): the fp64 norm, rounded once
        } else __syncthreads();
        ++cpt;
        FGW_PROF(7);  // T store + err
    }
    __syncthreads();
    for (int t = tid; t < NN; t += NT) { const int i = t / N, j = t - i * N; Tg[t] = Tl[i * P + j]; }
    if constexpr (PAIR) {
        int zero = 0;
        if constexpr (PPA) zero = __syncthreads_or(ppa_zero);
        if (tid == 0) { info[b * 4 + 0] = cpt; info[b * 4 + 1] = sk_total; info[b * 4 + 2] = zero ? 4 : 0; info[b * 4 + 3] = asym ? 0 : 1; }      // (asym: false without ASYM)
        return;
    }
    if constexpr (PPA) { if (__syncthreads_or(ppa_zero) && tid == 0) atomicOr(&info[b * 4 + 3], 4); }
    if (tid == 0) { atomicAdd(&info[b * 4 + 1], cpt); atomicAdd(&info[b * 4 + 2], sk_total); }
    FGW_PROF(8);      // T -> global
    // ---- contributions to the barycenter update (summed over s by k_fgw_update_parts)
    if (!prm.fixed_features) {                                          // Ypart = T @ Z                      (utils.py:90-95)
        fgw_part_t *Yp = Ypart + ((size_t)b * D.K + s) * N * d;
        mm_f64_glb<NW, false>(N, d, N, Mr, P, Z, d, [&](int i, int c, double v) { Yp[(size_t)i * d + c] = (fgw_part_t)v; });
    }
    FGW_PROF(9);      // Ypart = T @ Z
    if (!prm.fixed_structure) {                                         // Cpart = T @ C2 @ T^T               (utils.py:67-73)
        fgw_part_t *Cp = Cpart + ((size_t)b * D.K + s) * NN;
        if constexpr (KL)
            mm_f64<NW>(N, N, N, [&](int i, int k) { return (double)Tl[i * P + k]; },
                   [&](int k, int j) { const double cv = (double)C2[k * N + j]; return log(cv > 1e-15 ? cv : 1e-15); },
                   [&](int i, int j, double v) { Al[i * P + j] = v; });
        else
            mm_f64_glb<NW, false>(N, N, N, Mr, P, C2, N, [&](int i, int j, double v) { Al[i * P + j] = v; });
        __syncthreads();
        mm_f64_glb<NW, true>(N, N, N, Al, P, Mr, P, [&](int i, int j, double v) { Cp[i * N + j] = (fgw_part_t)v; });
    }
    FGW_PROF(10);     // Cpart = T @ C2 @ T^T
    FGW_PROF_FLUSH;
    };
    if constexpr (!SECOND) solve(blockIdx.x);
    else {      // one workgroup per 64 couplings: their flags are fetched by ONE load per lane (a ballot every wavefront forms for itself)
        const int total = D.B * D.K, base = (int)blockIdx.x * 64, l = (int)threadIdx.x & 63;
        unsigned long long m = __ballot(base + l < total && only[base + l < total ? base + l : 0] != 0);
        while (m) {
            const int k = __ffsll((long long)m) - 1;
            m &= m - 1;
            solve(base + k);
            __syncthreads();                                            // LDS is re-staged by the next trip
        }
    }
}
}  // namespace
