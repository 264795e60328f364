// The pair solve for gfx950: the reference's fgw(M, C1, C2, p, q, ...) (bregman.py:8-67 -> fgw_projected :70-167 / fgw_bregman :170-279) for B pairs of
// attributed graphs at once, one workgroup per pair, with the reference's log: the error list and fgw_dist (bregman.py:149-150, :163-164).
//   k_fgw_pair_init              C1 widened to fp64, errs <- NaN, info <- 0
//   k_fgw_coupling_pair          PGD / PPA: fgw_coupling_solve (fgw_coupling.h), the solve of k_fgw_coupling, with PAIR = true            (here)
//   k_fgw_coupling_bapg_pair     BAPG: the body of k_fgw_coupling_bapg (fgw_bapg_body.inc) compiled with PAIR = true                    (fgw_bapg.hip)
//   k_fgw_pair_dist              fgw_dist of the returned plan; also exported on its own (conan_fgw_pair_dist)
//   k_fgw_pair_dist_bwd          its gradient in M, C1, C2, p, q at a fixed plan (conan_fgw_pair_dist_bwd)
#include "fgw_coupling.h"
namespace {
// The pair form (what PAIR changes: in front of k_fgw_coupling, fgw.hip; DESIGN.md 3.3, "Pair form"), under the barycenter form's names: Ys = M and Cs = C2 [B,N,N], ps = q and pb = p [B,N] (nullable: uniform), Cw = the widened C1, Tw = T (in: G0
// when outer = 1 and prm.warmstart), D = {B, 1, N, 0, P}, y_zero = 1 | (symmetric=None) << 1.  What it has none of (Yw, active, Ypart, Cpart, only, adj) goes to the solve as constants.
template <int MODE, bool KL, int NW, bool PPA, bool ASYM>
__global__ void __launch_bounds__(64 * NW) k_fgw_coupling_pair(
    const float *__restrict__ Ys, const float *__restrict__ Cs, const float *__restrict__ ps, const float *__restrict__ pb,
    FgwDims D, conan_fgw_params prm, int outer, int y_zero, const double *__restrict__ Cw, float *__restrict__ Tw, int *__restrict__ info,
    char *__restrict__ scratch, FgwPair pr) {
    fgw_coupling_solve<MODE, KL, NW, false, PPA, ASYM, true>(Ys, Cs, ps, pb, D, prm, outer, y_zero, Cw, nullptr, nullptr, Tw, info, scratch, nullptr, nullptr, nullptr, FgwAdj{}, pr);
}
// conan_fgw_pair_fwd's first launch: C1 widened to fp64 (the operand type of the coupling kernels' products), errs filled with NaN, info zeroed
__global__ void __launch_bounds__(256) k_fgw_pair_init(const float *__restrict__ C1, double *__restrict__ C1w, int NN, float *__restrict__ errs, int nerr,
                                                       int *__restrict__ info) {
    const int b = blockIdx.x;
    for (int t = threadIdx.x; t < NN; t += 256) C1w[(size_t)b * NN + t] = (double)C1[(size_t)b * NN + t];
    for (int t = threadIdx.x; t < nerr; t += 256) errs[(size_t)b * nerr + t] = __builtin_nanf("");
    if (threadIdx.x < 4) info[b * 4 + threadIdx.x] = 0;
}

// fgw_dist of the reference's log (bregman.py:163-164, :272 with utils.py:4-64), one workgroup per pair:
//     (1 - alpha) sum_ij M_ij T_ij + alpha sum_ij (constC_ij - (h1(C1) T h2(C2)^T)_ij) T_ij,     constC_ij = sum_k f1(C1_ik) p_k + sum_k q_k f2(C2_jk)
// always from the problem itself, not its transpose (the reference does so after an asymmetric solve too).  The two products run on fp64 MFMA over
// blocks of R rows of A = C1 T held in LDS (R = N when the matrix fits).  Every sum is fp64, per thread in index order, then over the lanes and the
// wavefronts in a fixed order: no atomics, the same bits on every run and for every batch the pair is part of.
template <bool KL, int NW>
__global__ void __launch_bounds__(64 * NW) k_fgw_pair_dist(const float *__restrict__ M, const float *__restrict__ C1, const float *__restrict__ C2,
                                                           const float *__restrict__ p, const float *__restrict__ q, const float *__restrict__ T, int N,
                                                           int R, float alpha_f, float *__restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int NT = 64 * NW;
    const int b = blockIdx.x, P = fgw_pitch(N), NN = N * N;
    const int tid = threadIdx.x;
    double *pa = reinterpret_cast<double *>(smem), *qb = pa + N, *cc = pa + 2 * N, *rc = pa + 3 * N, *red = pa + 4 * N, *A = red + 16;      // A [R,P]
    M += (size_t)b * NN; C1 += (size_t)b * NN; C2 += (size_t)b * NN; T += (size_t)b * NN;
    const double alpha = (double)alpha_f;
    for (int i = tid; i < N; i += NT) {
        pa[i] = p ? (double)p[(size_t)b * N + i] : 1.0 / (double)N;
        qb[i] = q ? (double)q[(size_t)b * N + i] : 1.0 / (double)N;
    }
    __syncthreads();
    {   // init_matrix (utils.py:39-41): 8 lanes per index, as in the coupling kernels
        constexpr int LPI = 8;
        for (int i0 = 0; i0 < N; i0 += NT / LPI) {
            const int i = i0 + tid / LPI, sub = tid % LPI;
            double r1 = 0.0, r2 = 0.0;
            if (i < N)
                for (int k = sub; k < N; k += LPI) {
                    const double c1 = (double)C1[i * N + k], c2 = (double)C2[i * N + k];
                    r1 += (KL ? c1 * log(c1 + 1e-15) - c1 : c1 * c1) * pa[k];
                    r2 += qb[k] * (KL ? c2 : c2 * c2);
                }
#pragma unroll
            for (int o = 1; o < LPI; o <<= 1) { r1 += __shfl_xor(r1, o, 64); r2 += __shfl_xor(r2, o, 64); }
            if (i < N && sub == 0) { cc[i] = r1; rc[i] = r2; }
        }
    }
    __syncthreads();
    double lin = 0.0, quad = 0.0;                                         // sum M T ; sum (constC - G) T
    for (int t = tid; t < NN; t += NT) {
        const int i = t / N, j = t - i * N;
        const double tv = (double)T[t];
        lin += (double)M[t] * tv;
        quad += (cc[i] + rc[j]) * tv;
    }
    for (int r0 = 0; r0 < N; r0 += R) {
        const int rows = min(R, N - r0);
        mm_f64_glb<NW, false>(rows, N, N, C1 + (size_t)r0 * N, N, T, N, [&](int i, int j, double v) { A[i * P + j] = v; });      // A = h1(C1) T
        __syncthreads();
        auto take = [&](int i, int j, double g) { quad -= (KL ? 1.0 : 2.0) * g * (double)T[(r0 + i) * N + j]; };               // h2 = 2 C2: the 2 here
        if constexpr (KL)
            mm_f64<NW>(rows, N, N, [&](int i, int k) { return A[i * P + k]; }, [&](int k, int j) { return log((double)C2[j * N + k] + 1e-15); }, take);
        else
            mm_f64_glb<NW, true>(rows, N, N, A, P, C2, N, take);
        __syncthreads();
    }
    const double total = block_sum_d<NW>((1.0 - alpha) * lin + alpha * quad, red);
    if (tid == 0) out[b] = (float)total;
}

// The gradient of k_fgw_pair_dist's value at a FIXED plan T (the couplings are constants of the backward, as in fgw_grad.hip; DESIGN.md 3.3, "Pair
// form: backward"), one workgroup per pair, g = gout[b], r = T 1, c = T^T 1:
//     dM  = (1 - alpha) g T
//     dC1 = alpha g (f1'(C1) o (r p^T) - T h2(C2) T^T)        dp_k = alpha g sum_i f1(C1_ik) r_i
//     dC2 = alpha g (f2'(C2) o (c q^T) - (T^T C1 T) o h2'(C2))  dq_k = alpha g sum_j f2(C2_jk) c_j
// with f1, f2, h2 of init_matrix (utils.py:20-32): square a^2, b^2, 2b; KL a log(a + 1e-15) - a, b, log(b + 1e-15).  No symmetry of C1 / C2 is assumed.
// Each triple product is two fp64 MFMA products over blocks of R rows of the intermediate (T h2(C2) resp. T^T C1) held in LDS, the LDS layout of
// k_fgw_pair_dist; the elementwise terms ride in the second product's epilogue.  A null output is skipped with its products.  Every sum is fp64 in a
// fixed order, no atomics, nothing shared between workgroups: the same bits on every run and for every batch the pair is part of.
template <bool KL, int NW>
__global__ void __launch_bounds__(64 * NW) k_fgw_pair_dist_bwd(const float *__restrict__ C1, const float *__restrict__ C2, const float *__restrict__ p,
                                                               const float *__restrict__ q, const float *__restrict__ T, const float *__restrict__ gout,
                                                               int N, int R, float alpha_f, float *__restrict__ dM, float *__restrict__ dC1,
                                                               float *__restrict__ dC2, float *__restrict__ dp, float *__restrict__ dq) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int NT = 64 * NW;
    const int b = blockIdx.x, P = fgw_pitch(N), NN = N * N;
    const int tid = threadIdx.x;
    double *pa = reinterpret_cast<double *>(smem), *qb = pa + N, *rs = pa + 2 * N, *cs = pa + 3 * N, *A = pa + 4 * N + 16;      // A [R,P]
    C1 += (size_t)b * NN; C2 += (size_t)b * NN; T += (size_t)b * NN;
    const double g = (double)gout[b], ag = (double)alpha_f * g;
    for (int i = tid; i < N; i += NT) {
        pa[i] = p ? (double)p[(size_t)b * N + i] : 1.0 / (double)N;
        qb[i] = q ? (double)q[(size_t)b * N + i] : 1.0 / (double)N;
    }
    if (dC1 || dp) {                                                       // r = T 1: 8 lanes per row
        constexpr int LPI = 8;
        for (int i0 = 0; i0 < N; i0 += NT / LPI) {
            const int i = i0 + tid / LPI, sub = tid % LPI;
            double r = 0.0;
            if (i < N)
                for (int k = sub; k < N; k += LPI) r += (double)T[i * N + k];
#pragma unroll
            for (int o = 1; o < LPI; o <<= 1) r += __shfl_xor(r, o, 64);
            if (i < N && sub == 0) rs[i] = r;
        }
    }
    if (dC2 || dq)                                                         // c = T^T 1: one thread per column
        for (int j = tid; j < N; j += NT) {
            double c = 0.0;
            for (int i = 0; i < N; ++i) c += (double)T[i * N + j];
            cs[j] = c;
        }
    __syncthreads();
    if (dM) {
        const double s = (1.0 - (double)alpha_f) * g;
        for (int t = tid; t < NN; t += NT) dM[(size_t)b * NN + t] = (float)(s * (double)T[t]);
    }
    if (dp)
        for (int k = tid; k < N; k += NT) {
            double s = 0.0;
            for (int i = 0; i < N; ++i) {
                const double a = (double)C1[i * N + k];
                s += (KL ? a * log(a + 1e-15) - a : a * a) * rs[i];
            }
            dp[(size_t)b * N + k] = (float)(ag * s);
        }
    if (dq)
        for (int k = tid; k < N; k += NT) {
            double s = 0.0;
            for (int j = 0; j < N; ++j) {
                const double c2 = (double)C2[j * N + k];
                s += (KL ? c2 : c2 * c2) * cs[j];
            }
            dq[(size_t)b * N + k] = (float)(ag * s);
        }
    if (dC1) {
        dC1 += (size_t)b * NN;
        for (int r0 = 0; r0 < N; r0 += R) {
            const int rows = min(R, N - r0);
            auto keep = [&](int i, int j, double v) { A[i * P + j] = v; };                                                      // A = T C2 (h2's 2: in the epilogue) / T log(C2 + 1e-15)
            if constexpr (KL)
                mm_f64<NW>(rows, N, N, [&](int i, int k) { return (double)T[(r0 + i) * N + k]; }, [&](int k, int j) { return log((double)C2[k * N + j] + 1e-15); }, keep);
            else
                mm_f64_glb<NW, false>(rows, N, N, T + (size_t)r0 * N, N, C2, N, keep);
            __syncthreads();
            mm_f64_glb<NW, true>(rows, N, N, A, P, T, N, [&](int i, int j, double v) {
                const int at = (r0 + i) * N + j;
                const double a = (double)C1[at], w = rs[r0 + i] * pa[j];
                dC1[at] = (float)(ag * (KL ? (log(a + 1e-15) + a / (a + 1e-15) - 1.0) * w - v : 2.0 * (a * w - v)));
            });
            __syncthreads();
        }
    }
    if (dC2) {
        dC2 += (size_t)b * NN;
        for (int r0 = 0; r0 < N; r0 += R) {
            const int rows = min(R, N - r0);
            mm_f64<NW>(rows, N, N, [&](int j, int i) { return (double)T[i * N + r0 + j]; }, [&](int i, int k) { return (double)C1[i * N + k]; },
                       [&](int j, int k, double v) { A[j * P + k] = v; });                                                        // A = T^T C1
            __syncthreads();
            mm_f64_glb<NW, false>(rows, N, N, A, P, T, N, [&](int j, int l, double v) {
                const int at = (r0 + j) * N + l;
                const double c2 = (double)C2[at], w = cs[r0 + j] * qb[l];
                dC2[at] = (float)(ag * (KL ? w - v / (c2 + 1e-15) : 2.0 * (c2 * w - v)));
            });
            __syncthreads();
        }
    }
}

// The workspace of conan_fgw_pair_fwd, described once like fgw_workspace; total = 0 for what the entry point refuses.
FgwPairWorkspace fgw_pair_workspace(int B, int N, int solver, int symmetric) {
    FgwPairWorkspace w{};
    if (B <= 0 || N <= 0 || solver < 0 || solver > 2 || symmetric < -1 || symmetric > 1) return w;
    const size_t NN = (size_t)N * N, NP = (size_t)N * pitch_of(N);
    w.stride = solver == 2 ? conan_fgw_bapg_pair_stride(N, symmetric != 1) : coupling_scratch_stride(NP);
    size_t end = 0;
    auto region = [&](size_t bytes) { const size_t at = end; end += bytes; return at; };
    w.C1w = region(al256((size_t)B * NN * 8));
    w.scratch = region(al256((size_t)B * w.stride));
    w.total = end;
    return w;
}
// rows of A = C1 T that k_fgw_pair_dist holds in LDS at a time (0: not even 16 fit), and its dynamic LDS
inline int pair_dist_rows(int N, size_t *lds_bytes) {
    const size_t vec = (size_t)(4 * N + 16) * 8, row = (size_t)pitch_of(N) * 8;
    if (vec + 16 * row > LDS_LIMIT && vec + (size_t)N * row > LDS_LIMIT) return 0;
    const size_t fit = (LDS_LIMIT - vec) / row;
    const int R = fit >= (size_t)N ? N : (int)(fit / 16 * 16);
    *lds_bytes = vec + (size_t)R * row;
    return R;
}
int fgw_pair_dist_launch(const float *M, const float *C1, const float *C2, const float *p, const float *q, const float *T, int B, int N, float alpha,
                         int loss_fun, float *out, hipStream_t s) {
    size_t bytes = 0;
    const int R = pair_dist_rows(N, &bytes);
    if (R <= 0) return CONAN_E_UNSUPPORTED;
    if (loss_fun) launch_lds(k_fgw_pair_dist<true, GEN_NW>, B, 64 * GEN_NW, bytes, s, M, C1, C2, p, q, T, N, R, alpha, out);
    else launch_lds(k_fgw_pair_dist<false, GEN_NW>, B, 64 * GEN_NW, bytes, s, M, C1, C2, p, q, T, N, R, alpha, out);
    return CONAN_OK;
}
// the backward shares k_fgw_pair_dist's LDS layout (four fp64 vectors and R rows of an intermediate product), so also its R
int fgw_pair_dist_bwd_launch(const float *C1, const float *C2, const float *p, const float *q, const float *T, const float *gout, int B, int N, float alpha,
                             int loss_fun, float *dM, float *dC1, float *dC2, float *dp, float *dq, hipStream_t s) {
    size_t bytes = 0;
    const int R = pair_dist_rows(N, &bytes);
    if (R <= 0) return CONAN_E_UNSUPPORTED;
    if (loss_fun) launch_lds(k_fgw_pair_dist_bwd<true, GEN_NW>, B, 64 * GEN_NW, bytes, s, C1, C2, p, q, T, gout, N, R, alpha, dM, dC1, dC2, dp, dq);
    else launch_lds(k_fgw_pair_dist_bwd<false, GEN_NW>, B, 64 * GEN_NW, bytes, s, C1, C2, p, q, T, gout, N, R, alpha, dM, dC1, dC2, dp, dq);
    return CONAN_OK;
}
template <int MD>
void launch_pair(const FgwPairCall &c, size_t lds_bytes, int solver) {
    with_flags([&](auto KL, auto PPA, auto ASYM) {
        launch_lds(k_fgw_coupling_pair<MD, KL.value, GEN_NW, PPA.value, ASYM.value>, c.D.B, 64 * GEN_NW, lds_bytes, c.s, c.M, c.C2, c.q, c.p, c.D, c.prm,
                   c.warm, 1 | (c.symmetric < 0 ? 2 : 0), c.C1w, c.T, c.info, c.scratch, c.pr);
    }, c.prm.loss_fun != 0, solver == 1, c.symmetric != 1);
}

}  // namespace

extern "C" {

// ---- the pair solve: fgw(M, C1, C2, p, q) of bregman.py:8-279 for B pairs at once
long long conan_fgw_pair_workspace_bytes(int B, int N, int solver, int symmetric) { return (long long)fgw_pair_workspace(B, N, solver, symmetric).total; }

int conan_fgw_pair_dist(const float *M, const float *C1, const float *C2, const float *p, const float *q, const float *T, int B, int N, float alpha,
                        int loss_fun, float *out, void *stream) {
    if (!M || !C1 || !C2 || !T || !out || B <= 0 || N <= 0 || (loss_fun != 0 && loss_fun != 1)) return CONAN_E_BADARG;
    const int rc = fgw_pair_dist_launch(M, C1, C2, p, q, T, B, N, alpha, loss_fun, out, as_stream(stream));
    if (rc != CONAN_OK) return rc;
    CONAN_LAUNCH_CHECK();
    return CONAN_OK;
}

int conan_fgw_pair_dist_bwd(const float *C1, const float *C2, const float *p, const float *q, const float *T, const float *gout, int B, int N,
                            float alpha, int loss_fun, float *dM, float *dC1, float *dC2, float *dp, float *dq, void *stream) {
    if (!C1 || !C2 || !T || !gout || B <= 0 || N <= 0 || (loss_fun != 0 && loss_fun != 1)) return CONAN_E_BADARG;
    if ((!dM && !dC1 && !dC2 && !dp && !dq) || (dp && !p) || (dq && !q)) return CONAN_E_BADARG;
    const int rc = fgw_pair_dist_bwd_launch(C1, C2, p, q, T, gout, B, N, alpha, loss_fun, dM, dC1, dC2, dp, dq, as_stream(stream));
    if (rc != CONAN_OK) return rc;
    CONAN_LAUNCH_CHECK();
    return CONAN_OK;
}

int conan_fgw_pair_fwd(const float *M, const float *C1, const float *C2, const float *p, const float *q, const float *G0, int B, int N,
                       const conan_fgw_params *params, int solver, int symmetric, float *T, float *fgw_dist, int *info, float *errs, void *workspace,
                       void *stream) {
    if (solver < 0 || solver > 2 || symmetric < -1 || symmetric > 1) return CONAN_E_BADARG;
    if (!M || !C1 || !C2 || !params || !T || !info || !errs || !workspace || B <= 0 || N <= 0) return CONAN_E_BADARG;
    if (params->max_iter <= 0 || (solver != 2 && params->num_iter_max <= 0) || (params->loss_fun != 0 && params->loss_fun != 1)) return CONAN_E_BADARG;
    size_t dist_lds = 0;
    if (fgw_dist && pair_dist_rows(N, &dist_lds) <= 0) return CONAN_E_UNSUPPORTED;
    const FgwPairWorkspace w = fgw_pair_workspace(B, N, solver, symmetric);
    const size_t NN = (size_t)N * N;
    FgwPairCall c{};
    c.M = M; c.C2 = C2; c.p = p; c.q = q;
    c.C1w = ws_at<double>(workspace, w.C1w);
    c.D = FgwDims{B, 1, N, 0, pitch_of(N)};
    c.prm = *params;
    c.prm.inner_tol = params->tol;                              // the kernels' loop tests inner_tol: here the solve's own tol
    c.prm.warmstart = G0 ? 1 : 0;
    c.prm.fixed_structure = c.prm.fixed_features = 1;
    c.symmetric = symmetric; c.warm = G0 ? 1 : 0;
    c.T = T; c.info = info;
    c.pr = FgwPair{M, errs, (params->max_iter + 9) / 10};
    c.scratch = ws_at<char>(workspace, w.scratch); c.scratch_stride = w.stride;
    c.s = as_stream(stream);
    k_fgw_pair_init<<<B, 256, 0, c.s>>>(C1, ws_at<double>(workspace, w.C1w), (int)NN, errs, c.pr.nerr, info);
    if (G0) (void)hipMemcpyAsync(T, G0, (size_t)B * NN * sizeof(float), hipMemcpyDeviceToDevice, c.s);      // T0 = G0 through the warm-start branch
    if (solver == 2) conan_fgw_bapg_pair(c);
    else {
        size_t lds_bytes = 0;
        const int mode = general_mode(N, &lds_bytes);
        if (mode == 2) launch_pair<2>(c, lds_bytes, solver);
        else if (mode == 1) launch_pair<1>(c, lds_bytes, solver);
        else launch_pair<0>(c, lds_bytes, solver);
    }
    if (fgw_dist) (void)fgw_pair_dist_launch(M, C1, C2, p, q, T, B, N, params->alpha, params->loss_fun, fgw_dist, c.s);
    CONAN_LAUNCH_CHECK();
    return CONAN_OK;
}

}  // extern "C"
