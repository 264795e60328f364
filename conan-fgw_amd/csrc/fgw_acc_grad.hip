// The reference's gradient through the unrolled epochs of FGWMixup's coupling solve for gfx950: the backward of conan_fgw_acc_pair_fwd
// (fgw_acc.hip; the reference's fused_ACC_torch, barycenter.py:228-256, is plain differentiable torch) to M, A, Bm, a, b and the start X0, from the
// cotangents of the returned plan and of the FGWMixup distance of that plan (ops.fgw_acc_pair_distance's formula).  B pairs per launch, one
// workgroup of UNROLL_NW wavefronts per pair (conan_fgw_acc_pair_bwd; DESIGN.md 3.3, "FGWMixup: the unrolled gradient").
//
// Two steps, for the epochs the forward ran (info[b,0], read here, clamped to [0, epoch]):
//
// (1) Replay.  acc_epochs (fgw_acc_body.h, the forward's own text) runs those epochs again without objective checks and records the fp64 input
//     X_h of every half-step h = 0 .. 2 epochs - 1 (after the 1e-10 lift for even h) in the pair's slice of the workspace.  Its final X is the
//     forward's, bit for bit (X_chk).
// (2) Reverse walk.  With the cotangents dX (of the plan) and dd (of the distance), alpha' = 1 - alpha and c1 = (A o A) a 1^T + 1 b^T (Bm o Bm):
//         Gb = dX + dd (alpha' M + alpha c1 - 2 alpha (A X Bm + A^T X Bm^T))                    at the final X, and the direct partials
//         dM = dd alpha' X,   dA = dd alpha (2 A o (r a^T) - 2 X Bm^T X^T),   dBm = dd alpha (2 Bm o (b c^T) - 2 (A X)^T X),
//         da_k = dd alpha sum_i A_ik^2 r_i,   db_l = dd alpha sum_j Bm_lj^2 c_j,               r = X 1, c = X^T 1;
//     then for h = 2 epochs - 1 .. 0, X = X_h, w = b and lines = columns for odd h, w = a and lines = rows for even h:
//         G  = 4 alpha (A X) Bm - alpha' M      E = exp(G / rho)      Z = E o X      r = line sums of Z      X' = Z (w / r)
//         s  = line sums of Gb o X'             dw += s / w           dZ = (w / r) (Gb - s / w)
//         dG = dZ o Z / rho                     dM -= alpha' dG       H = dG Bm^T    Gb <- dZ o E + 4 alpha A^T H
//         dA += 4 alpha H X^T                   dBm += 4 alpha (A X)^T dG
//     (the lift passes Gb through), and at the end dX0 = Gb, or without a start da += Gb b, db += Gb^T a.
//
// Six N^3 products per half-step against the forward's two, all on fp64 MFMA: A X, (A X) Bm, H and H X^T through mm_f64_glb, the two whose LEFT
// operand is transposed (A^T H, (A X)^T dG) through the element-reader form mm_f64_pad.  dM, dA, dBm, da, db accumulate in fp64 over the whole
// walk and are rounded to fp32 once; every loop is bounded by `epoch`.  The conventions this kernel shares with its siblings (summation order,
// nodes without mass, NaN, storage) are stated once, in fgw_unroll.h, with the pieces the kernels can share.
//
// Nodes without mass (a_i = 0 or b_j = 0: how rectangular and own-size pairs are embedded): their entries of every X_h are exactly zero and
// constants of the solve, so Gb is held at zero there, their rows / columns of dM, dA, dBm and their da_i / db_j are written as exactly 0 (the
// reference divides by the weight: the same documented deviation as the unrolled Sinkhorn gradient's).  A pair whose forward raised flags bit 2 (a
// zero or non-finite line sum) gets NaN in every gradient, as the reference's autograd gives.
//
// Storage (fgw_unroll.h): the five matrices are X, AX, Gb, Z (then dG), E (then H).  The three accumulators dM, dA, dBm are touched once per
// half-step and live in the workspace at every size (in LDS they would lower the residency bound from 61 to 49).  The launch bound of 4 waves
// per SIMD holds the kernel at 128 VGPRs: two workgroups per CU.  The replay needs X, AX and alpha' M: it borrows Gb for the last.  Workspace per pair: (2 epoch + 3) N^2 * 8 bytes, + 5 N P * 8 outside LDS, rounded up to 256.
#include "fgw_acc_body.h"
#include "../../include/conan_fgw_hip_ext.h"

namespace {

struct AccBwdCall : UnrollPairIO {    // B = Bm, chk = X_chk
    int N, P, epoch;
    double alpha, rho;              // (fp64 from the host: the scalar unit has no fp64 conversions)
    char *ws;
    size_t ws_stride;               // bytes per pair
};

// vectors: a, b, sc, q, da, db, c1's two halves [N] each, and reduction space
using AccStore = UnrollStore<8, true>;
inline size_t accb_stride(int N, int epoch) { return AccStore::stride(N, ((size_t)2 * epoch + 3) * N * N * 8); }      // the record and the three accumulators

template <bool LDS>
__global__ void __launch_bounds__(64 * UNROLL_NW, 4) k_fgw_acc_pair_bwd(AccBwdCall c) {      // 4 waves per SIMD = two workgroups per CU: 128 VGPRs (131 without the bound)
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int NW = UNROLL_NW, NT = 64 * NW;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int N = c.N, P = c.P, NN = N * N;
    double *pa = reinterpret_cast<double *>(smem), *qb = pa + N, *sc = qb + N, *qv = sc + N, *dac = qv + N, *dbc = dac + N, *ca = dbc + N, *cb = ca + N;
    double *red = cb + N, *pm = red + 16;
    double *rec = reinterpret_cast<double *>(c.ws + (size_t)b * c.ws_stride);                  // X_0 .. X_(2 epoch - 1) [N,N] each
    double *dMa = rec + (size_t)2 * c.epoch * NN, *dAa = dMa + NN, *dBa = dAa + NN;
    double *X = LDS ? reinterpret_cast<double *>(smem + AccStore::vec_bytes(N)) : dBa + NN;
    double *AX = X + N * P, *Gb = AX + N * P, *Z = Gb + N * P, *E = Z + N * P;
    const float *Mg = c.M + (size_t)b * NN, *Ag = c.A + (size_t)b * NN, *Bg = c.B + (size_t)b * NN;
    const float *Xs = c.X0 ? c.X0 + (size_t)b * NN : nullptr, *dXg = c.dX ? c.dX + (size_t)b * NN : nullptr;
    const double alpha = c.alpha, om = 1.0 - alpha, four_alpha = 4.0 * alpha, two_alpha = 2.0 * alpha, inv_rho = 1.0 / c.rho;
    const int epochs = __builtin_amdgcn_readfirstlane(min(max(c.info[b * 4 + 0], 0), c.epoch));      // a corrupt info can neither leave the record nor lengthen a loop
    const bool flagged = (__builtin_amdgcn_readfirstlane(c.info[b * 4 + 2]) & 4) != 0;

    auto line_sums = [&](bool col, auto f, double *out) { unroll_line_sums(tid, lane, wave, N, P, pm, col, f, out); };
    auto live = [&](int i, int j) { return unroll_live(pa, qb, i, j); };
    for (int i = tid; i < N; i += NT) {
        pa[i] = c.a ? (double)c.a[(size_t)b * N + i] : 1.0 / (double)N;
        qb[i] = c.b ? (double)c.b[(size_t)b * N + i] : 1.0 / (double)N;
        dac[i] = 0.0; dbc[i] = 0.0;
    }
    __syncthreads();

    // ---- step 1: the forward's epochs again (its start, its alpha' M, its loop), every half-step's input to the record ----------------------
    for (int t = tid; t < NN; t += NT) {
        const int i = t / N, j = t - i * N;
        const double x0 = Xs ? (double)Xs[t] : pa[i] * qb[j];
        X[i * P + j] = live(i, j) ? x0 : 0.0;
        Gb[i * P + j] = (1.0 - alpha) * (double)Mg[t];
    }
    __syncthreads();
    {
        const AccProblem<float> q{Ag, Bg, alpha, c.rho, 0.0, epochs, nullptr};
        acc_epochs<false>(q, N, P, pa, qb, sc, pm, red, X, AX, Gb, [&](int h, const double *Xc) {
            double *r = rec + (size_t)h * NN;
            for (int t = tid; t < NN; t += NT) { const int i = t / N, j = t - i * N; r[t] = Xc[i * P + j]; }
        });
    }
    if (c.chk)
        for (int t = tid; t < NN; t += NT) { const int i = t / N, j = t - i * N; c.chk[(size_t)b * NN + t] = (float)X[i * P + j]; }
    if (flagged) {                                                          // (workgroup-uniform) the reference's autograd gives NaN: so do we, everywhere
        const float nan = __builtin_nanf("");
        for (int t = tid; t < NN; t += NT) {
            c.dM[(size_t)b * NN + t] = nan; c.dA[(size_t)b * NN + t] = nan; c.dB[(size_t)b * NN + t] = nan;
            if (c.dX0) c.dX0[(size_t)b * NN + t] = nan;
        }
        for (int i = tid; i < N; i += NT) {
            if (c.da) c.da[(size_t)b * N + i] = nan;
            if (c.db) c.db[(size_t)b * N + i] = nan;
        }
        return;
    }

    // ---- step 2a: the cotangent of the final X and the direct partials of the distance -------------------------------------------------------
    if (c.ddist) {                                                          // (workgroup-uniform)
        const double dd = (double)c.ddist[b];
        line_sums(false, [&](int, int, int o) { return X[o]; }, sc);           // r = X 1
        line_sums(true, [&](int, int, int o) { return X[o]; }, qv);            // c = X^T 1
        for (int i = tid; i < N; i += NT) {
            double s1 = 0.0, s2 = 0.0, s3 = 0.0, s4 = 0.0;
            for (int k = 0; k < N; ++k) {
                const double aik = (double)Ag[i * N + k], aki = (double)Ag[k * N + i], bki = (double)Bg[k * N + i], bik = (double)Bg[i * N + k];
                s1 += aik * aik * pa[k];                                    // c1's row half at i
                s2 += qb[k] * bki * bki;                                    // c1's column half at i
                s3 += aki * aki * sc[k];                                    // da_i
                s4 += bik * bik * qv[k];                                    // db_i
            }
            ca[i] = s1; cb[i] = s2;
            dac[i] = dd * alpha * s3; dbc[i] = dd * alpha * s4;
        }
        mm_f64_glb<NW, false>(N, N, N, Ag, N, X, P, [&](int i, int j, double v) { AX[i * P + j] = v; });
        mm_f64_glb<NW, true>(N, N, N, X, P, Bg, N, [&](int i, int j, double v) { Z[i * P + j] = v; });              // Y = X Bm^T
        __syncthreads();
        mm_f64_glb<NW, false>(N, N, N, AX, P, Bg, N, [&](int i, int j, double g) {
            const double dx = dXg ? (double)dXg[i * N + j] : 0.0;
            Gb[i * P + j] = live(i, j) ? dx + dd * (om * (double)Mg[i * N + j] + alpha * (ca[i] + cb[j]) - two_alpha * g) : 0.0;
        });
        mm_f64_glb<NW, true>(N, N, N, Z, P, X, P, [&](int i, int k, double v) {                                     // Y X^T
            dAa[i * N + k] = dd * alpha * (2.0 * (double)Ag[i * N + k] * pa[k] * sc[i] - 2.0 * v);
        });
        mm_f64_pad<NW>(N, N, N, [&](int l, int k) { return AX[k * P + l]; }, [&](int k, int j) { return X[k * P + j]; }, [&](int l, int j, double v) {
            dBa[l * N + j] = dd * alpha * (2.0 * (double)Bg[l * N + j] * qb[l] * qv[j] - 2.0 * v);                   // (A X)^T X
        });
        for (int t = tid; t < NN; t += NT) { const int i = t / N, j = t - i * N; dMa[t] = dd * om * X[i * P + j]; }
        __syncthreads();
        mm_f64_pad<NW>(N, N, N, [&](int i, int k) { return (double)Ag[k * N + i]; }, [&](int k, int j) { return Z[k * P + j]; }, [&](int i, int j, double v) {
            if (live(i, j)) Gb[i * P + j] -= two_alpha * dd * v;                                                      // A^T Y
        });
    } else {
        for (int t = tid; t < NN; t += NT) {
            const int i = t / N, j = t - i * N;
            Gb[i * P + j] = live(i, j) ? (double)dXg[t] : 0.0;
            dMa[t] = 0.0; dAa[t] = 0.0; dBa[t] = 0.0;
        }
    }
    __syncthreads();

    // ---- step 2b: the half-steps in reverse ----------------------------------------------------------------------------------------------------
    for (int h = 2 * epochs - 1; h >= 0; --h) {
        const bool col = (h & 1) != 0;
        const double *w = col ? qb : pa;
        double *dw = col ? dbc : dac;
        const double *xr = rec + (size_t)h * NN;
        for (int t = tid; t < NN; t += NT) { const int i = t / N, j = t - i * N; X[i * P + j] = xr[t]; }
        __syncthreads();
        mm_f64_glb<NW, false>(N, N, N, Ag, N, X, P, [&](int i, int j, double v) { AX[i * P + j] = v; });
        __syncthreads();
        mm_f64_glb<NW, false>(N, N, N, AX, P, Bg, N, [&](int i, int j, double g) {
            const double x = X[i * P + j], m = (1.0 - alpha) * (double)Mg[i * N + j];
            const double e = live(i, j) ? exp((four_alpha * g - m) * inv_rho) : 0.0;
            E[i * P + j] = e; Z[i * P + j] = e * x;
        });
        __syncthreads();
        line_sums(col, [&](int, int, int o) { return Z[o]; }, sc);              // r
        line_sums(col, [&](int, int, int o) { return Gb[o] * Z[o]; }, qv);      // sum of Gb o Z: s = (w / r) times it
        for (int l = tid; l < N; l += NT) {
            const double wl = w[l];
            const double f = wl > 0.0 ? wl / sc[l] : 0.0, s = f * qv[l], q = wl > 0.0 ? s / wl : 0.0;
            dw[l] += q; sc[l] = f; qv[l] = q;
        }
        __syncthreads();
        for (int t = tid; t < NN; t += NT) {
            const int i = t / N, j = t - i * N, o = i * P + j, l = col ? j : i;
            const double dz = sc[l] * (Gb[o] - qv[l]), dg = dz * Z[o] * inv_rho;
            Gb[o] = dz * E[o];                                              // (E is 0 at a massless entry: Gb stays 0 there)
            Z[o] = dg;
            dMa[t] -= om * dg;
        }
        __syncthreads();
        mm_f64_glb<NW, true>(N, N, N, Z, P, Bg, N, [&](int i, int j, double v) { E[i * P + j] = v; });             // H = dG Bm^T
        __syncthreads();
        mm_f64_pad<NW>(N, N, N, [&](int i, int k) { return (double)Ag[k * N + i]; }, [&](int k, int j) { return E[k * P + j]; }, [&](int i, int j, double v) {
            if (live(i, j)) Gb[i * P + j] += four_alpha * v;                                                          // A^T H
        });
        mm_f64_glb<NW, true>(N, N, N, E, P, X, P, [&](int i, int k, double v) { dAa[i * N + k] += four_alpha * v; });       // H X^T
        mm_f64_pad<NW>(N, N, N, [&](int l, int k) { return AX[k * P + l]; }, [&](int k, int j) { return Z[k * P + j]; },
                       [&](int l, int j, double v) { dBa[l * N + j] += four_alpha * v; });                            // (A X)^T dG
        __syncthreads();
    }

    // ---- the start: its own gradient, or through a b^T to the weights ------------------------------------------------------------------------
    if (!Xs) {
        unroll_start_sums(tid, lane, wave, N, P, pm, Gb, pa, qb, sc, qv);
        for (int i = tid; i < N; i += NT) { dac[i] += sc[i]; dbc[i] += qv[i]; }
        __syncthreads();
    }
    for (int t = tid; t < NN; t += NT) {
        const int i = t / N, j = t - i * N;
        c.dM[(size_t)b * NN + t] = live(i, j) ? (float)dMa[t] : 0.f;
        c.dA[(size_t)b * NN + t] = (pa[i] > 0.0 && pa[j] > 0.0) ? (float)dAa[t] : 0.f;
        c.dB[(size_t)b * NN + t] = (qb[i] > 0.0 && qb[j] > 0.0) ? (float)dBa[t] : 0.f;
        if (c.dX0) c.dX0[(size_t)b * NN + t] = live(i, j) ? (float)Gb[i * P + j] : 0.f;
    }
    for (int i = tid; i < N; i += NT) {
        if (c.da) c.da[(size_t)b * N + i] = pa[i] > 0.0 ? (float)dac[i] : 0.f;
        if (c.db) c.db[(size_t)b * N + i] = qb[i] > 0.0 ? (float)dbc[i] : 0.f;
    }
}

}  // namespace

extern "C" {

int conan_fgw_acc_pair_bwd_lds_resident(int N) { return N > 0 && AccStore::resident(N) ? 1 : 0; }

long long conan_fgw_acc_pair_bwd_workspace_bytes(int B, int N, int epoch) {
    if (B <= 0 || epoch <= 0 || !AccStore::supported(N)) return 0;
    return (long long)((size_t)B * accb_stride(N, epoch));
}

int conan_fgw_acc_pair_bwd(const float *M, const float *A, const float *Bm, const float *a, const float *b, const float *X0, int B, int N, double alpha,
                           double rho, int epoch, const int *info, const float *dX, const float *ddist, float *dM, float *dA, float *dBm, float *da,
                           float *db, float *dX0, float *X_chk, void *workspace, void *stream) {
    AccBwdCall c{};
    static_cast<UnrollPairIO &>(c) = {M, A, Bm, a, b, X0, info, dX, ddist, dM, dA, dBm, da, db, dX0, X_chk};
    if (epoch <= 0 || unroll_pair_args(c, B, N, workspace, rho, alpha) != CONAN_OK) return CONAN_E_BADARG;
    if (!AccStore::supported(N)) return CONAN_E_UNSUPPORTED;
    c.N = N; c.P = pitch_of(N); c.epoch = epoch; c.alpha = alpha; c.rho = rho;
    c.ws = static_cast<char *>(workspace); c.ws_stride = accb_stride(N, epoch);
    if (AccStore::resident(N)) launch_lds(k_fgw_acc_pair_bwd<true>, B, 64 * UNROLL_NW, AccStore::lds_bytes(N), as_stream(stream), c);
    else launch_lds(k_fgw_acc_pair_bwd<false>, B, 64 * UNROLL_NW, AccStore::lds_bytes(N), as_stream(stream), c);
    CONAN_LAUNCH_CHECK();
    return CONAN_OK;
}

}  // extern "C"
