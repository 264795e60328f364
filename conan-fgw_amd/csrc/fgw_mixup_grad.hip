// The reference's gradient of the FGWMixup barycenter for gfx950: the backward of conan_fgw_mixup_barycenter_fwd (fgw_acc.hip; the reference's
// fgw_barycenters_BAPG, barycenter.py:259-390, runs its coupling solves with autograd on) through every epoch of every coupling solve of every
// outer iteration, to Ys, Cs, ps, p, lambdas and the starts init_C / init_Y, from the cotangents of the returned Y and C
// (conan_fgw_mixup_barycenter_bwd; DESIGN.md 3.3, "FGWMixup barycenter: the unrolled gradient").
//
// The forward's state (C_t, Y_t), t = 0 .. n (n = info[b,0], read here, clamped to [0, max_iter]), comes from the record that
// conan_fgw_mixup_barycenter_fwd_record keeps in fp64.  From (Yb_n, Cb_n) = the caller's cotangents, for t = n - 1 .. 0, TWO launches:
//
// k_fgw_mixup_bwd_coupling, one workgroup of UNROLL_NW wavefronts per coupling (b, s); a molecule with n <= t leaves at once:
//   (1) Replay.  M_s from Y_t as k_fgw_acc_coupling forms it, then acc_epochs (fgw_acc_body.h, the forward's own text, AccProblem<double>, WITH
//       its objective checks: the forward kept only the sum of the epoch counts, so the replay stops where the forward's rule stops) from
//       p ps_s^T, recording the fp64 input of every half-step.  Its final X_s is the forward's plan of that iteration bit for bit (T_chk for
//       the last one), its count goes to epochs_chk.
//   (2) The update steps Y_t+1 = diag(1/p) sum_s lam_s X_s Ys_s, C_t+1 = sum_s lam_s X_s h(Cs_s) X_s^T / (p p^T) (kl: exp of it, h = log
//       max(., 1e-15)).  With U = Yb_t+1 / p, V = Cb_t+1 / (p p^T) (kl: Cb_t+1 o C_t+1 / (p p^T)) and G = X_s^T V X_s:
//           Xb_s = lam_s (U Ys_s^T + V X_s h^T + V^T X_s h)      dYs_s += lam_s X_s^T U      dCs_s += lam_s G o h'      dlam_s += <U, X_s Ys_s> + <G, h>
//       (h' = 1, or 1 / Cs_s where Cs_s >= 1e-15 and 0 elsewhere: torch.clamp's mask).  Nothing of it under fixed_features / fixed_structure.
//   (3) The reverse walk of fgw_acc_grad.hip over the recorded half-steps, driven by Gb = Xb_s: dM_s; dA_s, this coupling's share of Cb_t;
//       dB_s, added to dCs_s; da, its share of dp; db, added to dps_s; the start p ps_s^T passes its gradient to da and db.
//   (4) The feature cost M_s = clamp(|y_i|^2 + |z_j|^2 - 2 y_i.z_j, 0), gradient passed where the unclamped value is >= 0 (torch.clamp):
//           Yb_t share = 2 (diag(rowsum dM_s) Y_t - dM_s Ys_s)      dYs_s += 2 (diag(colsum dM_s) Ys_s - dM_s^T Y_t)
// k_fgw_mixup_bwd_reduce, one workgroup per molecule: the update steps' direct partial in p,
//           dp_i -= (Yb_t+1,i . Y_t+1,i + sum_j (W_ij + W_ji)) / p_i,   W = Cb_t+1 o C_t+1 (kl: o log C_t+1),
//   then Cb_t, Yb_t and dp from the couplings' shares, s ascending.  Under fixed_structure / fixed_features C_t / Y_t is init_C / init_Y at
//   every t and Cb_t / Yb_t is Cb_t+1 / Yb_t+1 plus the shares.
// After t = 0, k_fgw_mixup_bwd_final rounds every output to fp32 once (Cb_0 -> dinit_C, Yb_0 -> dinit_Y) and sums dlambdas over the molecules,
// b ascending.  2 max_iter + 1 launches; every sum has a fixed order, there are no atomics; dYs_s, dCs_s, dps_s and the molecule's share of
// dlam_s are fp64 accumulators owned by the coupling's workgroup across all outer iterations; every loop is bounded by epoch / max_iter.
//
// The reverse walk is a SECOND COPY of fgw_acc_grad.hip's, with A read from the fp64 state and (1 - alpha) M from the workspace: moved into a
// shared header (three factorings tried, fgw_unroll.h) k_fgw_acc_pair_bwd no longer compiled to the parent's instructions or registers.
//
// Nodes without mass (p_i = 0, ps_sj = 0: how other sizes are embedded) get exactly 0 everywhere.  A molecule whose forward raised flags bit 2
// gets NaN in all its gradients and, through the sum over molecules, in dlambdas.
//
// Storage and the conventions shared with the sibling kernels: fgw_unroll.h.  The five matrices are X, AX, Gb, Z, E
// (conan_fgw_mixup_barycenter_bwd_lds_resident, N <= 61); the record, the accumulators and the shares live in the workspace at every size.
// The half-step record is reused by every outer iteration.
#include "fgw_acc_body.h"
#include "../../include/conan_fgw_hip_mixup_grad.h"

namespace {

// vectors: a, b, sc, q, da, db, |y_i|^2, |z_j|^2 [N] each, and reduction space
using MixStore = UnrollStore<8, true>;

// Byte offsets of the workspace's regions, in this order, and the total the size query returns.
struct MixWs {
    size_t Cbar, Ybar, dpacc;                                       // per molecule: [B,N,N], [B,N,d], [B,N]
    size_t Apart, Ypart, dppart, dCsacc, dYsacc, dpsacc, dlamacc;   // per coupling: [BK,N,N], [BK,N,d], [BK,N], [BK,N,N], [BK,N,d], [BK,N], [BK]
    size_t dM, Mraw, rec, mats;                                     // per coupling: [BK,N,N] x 2, [BK,2 epoch,N,N], outside LDS [BK,5,N,P]
    size_t total;
};
MixWs mix_workspace(int B, int K, int N, int d, int epoch) {
    MixWs w{};
    if (B <= 0 || K <= 0 || d <= 0 || epoch <= 0 || !MixStore::supported(N)) return w;
    const size_t NN = (size_t)N * N, Nd = (size_t)N * d, BK = (size_t)B * K;
    size_t end = 0;
    auto region = [&](size_t doubles) { const size_t at = end; end += al256(doubles * 8); return at; };
    w.Cbar = region(B * NN); w.Ybar = region(B * Nd); w.dpacc = region((size_t)B * N);
    w.Apart = region(BK * NN); w.Ypart = region(BK * Nd); w.dppart = region(BK * N);
    w.dCsacc = region(BK * NN); w.dYsacc = region(BK * Nd); w.dpsacc = region(BK * N); w.dlamacc = region(BK);
    w.dM = region(BK * NN); w.Mraw = region(BK * NN);
    w.rec = region(BK * 2 * (size_t)epoch * NN);
    w.mats = region(MixStore::resident(N) ? 0 : BK * 5 * (size_t)N * pitch_of(N));
    w.total = end;
    return w;
}

struct MixBwdCall {
    const float *Ys, *Cs, *ps, *p, *lambdas;
    const int *info;
    const double *Crec, *Yrec;      // [max_iter + 1][B][N,N], [max_iter + 1][B][N,d]: the forward's state after init and after every update
    const float *dY, *dC;           // the caller's cotangents (nullable)
    float *dYs, *dCs, *dps, *dp, *dlambdas, *dinit_C, *dinit_Y, *Tchk;
    int *epochs_chk;
    int B, K, N, d, P, epoch, max_iter, kl, fs, ff, has_init_Y;
    double alpha, rho, eps;         // (fp64 from the host: the scalar unit has no fp64 conversions)
    char *ws;
    MixWs w;
};

__device__ __forceinline__ double *mix_at(const MixBwdCall &c, size_t offset) { return reinterpret_cast<double *>(c.ws + offset); }
// the outer iterations molecule b ran; a corrupt info can neither leave the record nor lengthen a loop
__device__ __forceinline__ int mix_outer(const MixBwdCall &c, int b) { return __builtin_amdgcn_readfirstlane(min(max(c.info[b * 4 + 0], 0), c.max_iter)); }
__device__ __forceinline__ bool mix_flagged(const MixBwdCall &c, int b) { return (__builtin_amdgcn_readfirstlane(c.info[b * 4 + 3]) & 4) != 0; }

// Cb_t+1 / Yb_t+1 of molecule b at flat index t: the caller's cotangent in the molecule's first backward step, else what the reduce kernel left
__device__ __forceinline__ double mix_cbar(const MixBwdCall &c, bool first, int b, int t) {
    const size_t at = (size_t)b * c.N * c.N + t;
    return first ? (c.dC ? (double)c.dC[at] : 0.0) : mix_at(c, c.w.Cbar)[at];
}
__device__ __forceinline__ double mix_ybar(const MixBwdCall &c, bool first, int b, int t) {
    const size_t at = (size_t)b * c.N * c.d + t;
    return first ? (c.dY ? (double)c.dY[at] : 0.0) : mix_at(c, c.w.Ybar)[at];
}

template <bool LDS>
__global__ void __launch_bounds__(64 * UNROLL_NW, 4) k_fgw_mixup_bwd_coupling(MixBwdCall c, int t_out) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int NW = UNROLL_NW, NT = 64 * NW;
    const int cid = blockIdx.x, b = cid / c.K, s = cid - b * c.K;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int N = c.N, P = c.P, d = c.d, NN = N * N, Nd = N * d, B = c.B, K = c.K;
    const int n_out = mix_outer(c, b);
    if (t_out >= n_out || mix_flagged(c, b)) {                              // (workgroup-uniform) done earlier, or NaN everywhere (the final kernel writes it)
        if (c.epochs_chk && tid == 0) c.epochs_chk[((size_t)t_out * B + b) * K + s] = 0;
        return;
    }
    const bool first = t_out == n_out - 1;
    double *pa = reinterpret_cast<double *>(smem), *qb = pa + N, *sc = qb + N, *qv = sc + N, *dac = qv + N, *dbc = dac + N, *y2a = dbc + N, *z2a = y2a + N;
    double *red = z2a + N, *pm = red + 16;
    double *rec = mix_at(c, c.w.rec) + (size_t)cid * 2 * c.epoch * NN;      // X_0 .. X_(2 epoch - 1) [N,N] each
    double *dMa = mix_at(c, c.w.dM) + (size_t)cid * NN, *Mraw = mix_at(c, c.w.Mraw) + (size_t)cid * NN;
    double *dAa = mix_at(c, c.w.Apart) + (size_t)cid * NN, *dBa = mix_at(c, c.w.dCsacc) + (size_t)cid * NN;
    double *Yp = mix_at(c, c.w.Ypart) + (size_t)cid * Nd, *dYa = mix_at(c, c.w.dYsacc) + (size_t)cid * Nd;
    double *dpp = mix_at(c, c.w.dppart) + (size_t)cid * N, *dpsa = mix_at(c, c.w.dpsacc) + (size_t)cid * N, *dla = mix_at(c, c.w.dlamacc) + cid;
    double *X = LDS ? reinterpret_cast<double *>(smem + MixStore::vec_bytes(N)) : mix_at(c, c.w.mats) + (size_t)cid * 5 * N * P;
    double *AX = X + N * P, *Gb = AX + N * P, *Z = Gb + N * P, *E = Z + N * P;
    const float *Zg = c.Ys + (size_t)cid * Nd, *Bg = c.Cs + (size_t)cid * NN;
    const double *C0 = c.Crec + ((size_t)t_out * B + b) * NN, *C1 = c.Crec + ((size_t)(t_out + 1) * B + b) * NN;
    const double *Y0 = c.Yrec + ((size_t)t_out * B + b) * Nd;
    const double alpha = c.alpha, om = 1.0 - alpha, four_alpha = 4.0 * alpha, inv_rho = 1.0 / c.rho;
    const double lam = c.lambdas ? (double)c.lambdas[s] : 1.0 / (double)K;
    const int y_zero = (t_out == 0 && !c.has_init_Y) ? 1 : 0;

    auto line_sums = [&](bool col, auto f, double *out) { unroll_line_sums(tid, lane, wave, N, P, pm, col, f, out); };

    // ---- step 1: the forward's coupling solve of this outer iteration again (k_fgw_acc_coupling's text up to acc_epochs), recorded -----------
    for (int i = tid; i < N; i += NT) {
        pa[i] = c.p ? (double)c.p[(size_t)b * N + i] : 1.0 / (double)N;
        qb[i] = c.ps ? (double)c.ps[((size_t)b * K + s) * N + i] : 1.0 / (double)N;
        dac[i] = 0.0; dbc[i] = 0.0;
    }
    {   // 8 lanes per index, strided partial sums combined by xor-shuffles (fixed order)
        constexpr int LPI = 8;
        for (int i0 = 0; i0 < N; i0 += NT / LPI) {
            const int i = i0 + tid / LPI, sub = tid % LPI;
            double y2 = 0.0, z2 = 0.0;
            if (i < N)
                for (int k = sub; k < d; k += LPI) {
                    const double yy = Y0[i * d + k], zz = (double)Zg[i * d + k];
                    y2 += yy * yy; z2 += zz * zz;
                }
#pragma unroll
            for (int o = 1; o < LPI; o <<= 1) { y2 += __shfl_xor(y2, o, 64); z2 += __shfl_xor(z2, o, 64); }
            if (i < N && sub == 0) { y2a[i] = y2; z2a[i] = z2; }
        }
    }
    __syncthreads();
    auto live = [&](int i, int j) { return unroll_live(pa, qb, i, j); };
    double *Mb = Gb;                                                        // (1 - alpha) M: the replay borrows Gb for it
    for (int t = tid; t < NN; t += NT) { const int i = t / N, j = t - i * N; X[i * P + j] = pa[i] * qb[j]; }
    if (!y_zero) mm_f64_glb<NW, true>(N, N, d, Y0, d, Zg, d, [&](int i, int j, double v) { Mb[i * P + j] = v; });
    __syncthreads();
    for (int t = tid; t < NN; t += NT) {
        const int i = t / N, j = t - i * N;
        double m = -2.0 * (y_zero ? 0.0 : Mb[i * P + j]);
        m += y2a[i]; m += z2a[j];
        Mraw[t] = m;                                                        // unclamped: the walk clamps it again, step 4 reads the mask off it
        m = m > 0.0 ? m : 0.0;
        Mb[i * P + j] = (1.0 - alpha) * m;
    }
    __syncthreads();
    int epochs;
    {
        const AccProblem<double> q{C0, Bg, alpha, c.rho, c.eps, c.epoch, nullptr};
        const AccResult r = acc_epochs(q, N, P, pa, qb, sc, pm, red, X, AX, Mb, [&](int h, const double *Xc) {
            double *rh = rec + (size_t)h * NN;
            for (int t = tid; t < NN; t += NT) { const int i = t / N, j = t - i * N; rh[t] = Xc[i * P + j]; }
        });
        epochs = __builtin_amdgcn_readfirstlane(min(max(r.epochs, 0), c.epoch));
    }
    if (c.epochs_chk && tid == 0) c.epochs_chk[((size_t)t_out * B + b) * K + s] = epochs;
    if (c.Tchk && first)
        for (int t = tid; t < NN; t += NT) { const int i = t / N, j = t - i * N; c.Tchk[(size_t)cid * NN + t] = (float)X[i * P + j]; }

    // ---- step 2: the update steps at X = X_s: Gb = Xb_s and the direct partials -----------------------------------------------------------------
    for (int i = tid; i < N; i += NT) sc[i] = pa[i] > 0.0 ? 1.0 / pa[i] : 0.0;            // 1 / p, 0 at a node without mass
    for (int t = tid; t < NN; t += NT) {
        const int i = t / N, j = t - i * N;
        const double cv = (double)Bg[t];
        E[i * P + j] = c.kl ? log(cv > 1e-15 ? cv : 1e-15) : cv;                          // h(Cs_s)
        Gb[i * P + j] = 0.0;
        dMa[t] = 0.0; dAa[t] = 0.0;
        if (first) dBa[t] = 0.0;
    }
    if (first) {
        for (int t = tid; t < Nd; t += NT) dYa[t] = 0.0;
        for (int i = tid; i < N; i += NT) dpsa[i] = 0.0;
    }
    __syncthreads();
    auto U = [&](int i, int k) { return mix_ybar(c, first, b, i * d + k) * sc[i]; };
    auto V = [&](int i, int j) { return mix_cbar(c, first, b, i * N + j) * (c.kl ? C1[i * N + j] : 1.0) * (sc[i] * sc[j]); };
    double part = 0.0;
    if (!c.fs) {                                                            // (workgroup-uniform)
        mm_f64_pad<NW>(N, N, N, V, [&](int k, int j) { return X[k * P + j]; }, [&](int i, int j, double v) { AX[i * P + j] = v; });            // V X
        mm_f64_pad<NW>(N, N, N, [&](int i, int k) { return V(k, i); }, [&](int k, int j) { return X[k * P + j]; },
                       [&](int i, int j, double v) { Z[i * P + j] = v; });                                                                      // V^T X
        __syncthreads();
        mm_f64_glb<NW, true>(N, N, N, AX, P, E, P, [&](int i, int j, double v) { Gb[i * P + j] = lam * v; });                                 // (V X) h^T
        mm_f64_pad<NW>(N, N, N, [&](int l, int k) { return X[k * P + l]; }, [&](int k, int j) { return AX[k * P + j]; }, [&](int l, int j, double v) {
            const double cv = (double)Bg[l * N + j];
            dBa[l * N + j] += lam * v * (c.kl ? (cv >= 1e-15 ? 1.0 / cv : 0.0) : 1.0);                                                          // G o h'
            part += v * E[l * P + j];
        });
        __syncthreads();
        mm_f64_glb<NW, false>(N, N, N, Z, P, E, P, [&](int i, int j, double v) { Gb[i * P + j] += lam * v; });                                // (V^T X) h
        __syncthreads();
    }
    if (!c.ff) {
        mm_f64_pad<NW>(N, N, d, U, [&](int k, int j) { return (double)Zg[j * d + k]; }, [&](int i, int j, double v) { Gb[i * P + j] += lam * v; });     // U Ys^T
        mm_f64_pad<NW>(N, d, N, [&](int l, int k) { return X[k * P + l]; }, U, [&](int l, int k, double v) { dYa[l * d + k] += lam * v; });              // X^T U
        mm_f64_glb<NW, false>(N, d, N, X, P, Zg, d, [&](int i, int k, double v) { part += U(i, k) * v; });                                            // <U, X Ys>
        __syncthreads();
    }
    part = block_sum_d<NW>(part, red);
    if (tid == 0) *dla = (first ? 0.0 : *dla) + part;
    for (int t = tid; t < NN; t += NT) { const int i = t / N, j = t - i * N; if (!live(i, j)) Gb[i * P + j] = 0.0; }
    __syncthreads();

    // ---- step 3: the half-steps in reverse (fgw_acc_grad.hip's walk; A = C_t in fp64, (1 - alpha) M from the unclamped cost kept above) ---------
    for (int h = 2 * epochs - 1; h >= 0; --h) {
        const bool col = (h & 1) != 0;
        const double *w = col ? qb : pa;
        double *dw = col ? dbc : dac;
        const double *xr = rec + (size_t)h * NN;
        for (int t = tid; t < NN; t += NT) { const int i = t / N, j = t - i * N; X[i * P + j] = xr[t]; }
        __syncthreads();
        mm_f64_glb<NW, false>(N, N, N, C0, N, X, P, [&](int i, int j, double v) { AX[i * P + j] = v; });
        __syncthreads();
        mm_f64_glb<NW, false>(N, N, N, AX, P, Bg, N, [&](int i, int j, double g) {
            const double x = X[i * P + j], mr = Mraw[i * N + j], m = (1.0 - alpha) * (mr > 0.0 ? mr : 0.0);
            const double e = live(i, j) ? exp((four_alpha * g - m) * inv_rho) : 0.0;
            E[i * P + j] = e; Z[i * P + j] = e * x;
        });
        __syncthreads();
        line_sums(col, [&](int, int, int o) { return Z[o]; }, sc);              // r
        line_sums(col, [&](int, int, int o) { return Gb[o] * Z[o]; }, qv);      // sum of Gb o Z: s = (w / r) times it
        for (int l = tid; l < N; l += NT) {
            const double wl = w[l];
            const double f = wl > 0.0 ? wl / sc[l] : 0.0, sv = f * qv[l], q = wl > 0.0 ? sv / wl : 0.0;
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
        mm_f64_pad<NW>(N, N, N, [&](int i, int k) { return C0[k * N + i]; }, [&](int k, int j) { return E[k * P + j]; }, [&](int i, int j, double v) {
            if (live(i, j)) Gb[i * P + j] += four_alpha * v;                                                          // A^T H
        });
        mm_f64_glb<NW, true>(N, N, N, E, P, X, P, [&](int i, int k, double v) { dAa[i * N + k] += four_alpha * v; });       // H X^T
        mm_f64_pad<NW>(N, N, N, [&](int l, int k) { return AX[k * P + l]; }, [&](int k, int j) { return Z[k * P + j]; },
                       [&](int l, int j, double v) { dBa[l * N + j] += four_alpha * v; });                            // (A X)^T dG
        __syncthreads();
    }
    // the start p ps_s^T passes its gradient to the weights
    unroll_start_sums(tid, lane, wave, N, P, pm, Gb, pa, qb, sc, qv);
    for (int i = tid; i < N; i += NT) {
        dpp[i] = pa[i] > 0.0 ? dac[i] + sc[i] : 0.0;
        dpsa[i] += qb[i] > 0.0 ? dbc[i] + qv[i] : 0.0;
    }

    // ---- step 4: the feature cost, through the clamp -------------------------------------------------------------------------------------------
    for (int t = tid; t < NN; t += NT) { const int i = t / N, j = t - i * N; Z[i * P + j] = Mraw[t] >= 0.0 ? dMa[t] : 0.0; }
    __syncthreads();
    line_sums(false, [&](int, int, int o) { return Z[o]; }, sc);
    line_sums(true, [&](int, int, int o) { return Z[o]; }, qv);
    mm_f64_glb<NW, false>(N, d, N, Z, P, Zg, d, [&](int i, int k, double v) { Yp[i * d + k] = 2.0 * (sc[i] * Y0[i * d + k] - v); });
    mm_f64_pad<NW>(N, d, N, [&](int j, int k) { return Z[k * P + j]; }, [&](int k, int e) { return Y0[k * d + e]; },
                   [&](int j, int e, double v) { dYa[j * d + e] += 2.0 * (qv[j] * (double)Zg[j * d + e] - v); });
}

// Cb_t, Yb_t and dp of molecule b from the couplings' shares and the update steps' direct partial in p
__global__ void __launch_bounds__(256) k_fgw_mixup_bwd_reduce(MixBwdCall c, int t_out) {
    const int b = blockIdx.x, tid = threadIdx.x, NT = 256;
    const int N = c.N, d = c.d, NN = N * N, Nd = N * d, K = c.K, B = c.B;
    const int n_out = mix_outer(c, b);
    if (t_out >= n_out || mix_flagged(c, b)) return;
    const bool first = t_out == n_out - 1;
    const double *C1 = c.Crec + ((size_t)(t_out + 1) * B + b) * NN, *Y1 = c.Yrec + ((size_t)(t_out + 1) * B + b) * Nd;
    double *Cbar = mix_at(c, c.w.Cbar) + (size_t)b * NN, *Ybar = mix_at(c, c.w.Ybar) + (size_t)b * Nd, *dpa = mix_at(c, c.w.dpacc) + (size_t)b * N;
    const double *Ap = mix_at(c, c.w.Apart) + (size_t)b * K * NN, *Ypt = mix_at(c, c.w.Ypart) + (size_t)b * K * Nd;
    const double *dpp = mix_at(c, c.w.dppart) + (size_t)b * K * N;
    auto pw = [&](int i) { return c.p ? (double)c.p[(size_t)b * N + i] : 1.0 / (double)N; };
    for (int i = tid; i < N; i += NT) {
        double acc = 0.0;
        if (!c.ff)
            for (int k = 0; k < d; ++k) acc += mix_ybar(c, first, b, i * d + k) * Y1[i * d + k];
        if (!c.fs)
            for (int j = 0; j < N; ++j) {
                const double cij = C1[i * N + j], cji = C1[j * N + i];
                double wij = mix_cbar(c, first, b, i * N + j) * cij, wji = mix_cbar(c, first, b, j * N + i) * cji;
                if (c.kl) {                                                 // W o log C; an underflowed C (W = 0) contributes 0, not 0 * -inf
                    wij = wij != 0.0 ? wij * log(cij) : 0.0;
                    wji = wji != 0.0 ? wji * log(cji) : 0.0;
                }
                acc += wij + wji;
            }
        const double pi = pw(i);
        double v = (first ? 0.0 : dpa[i]) + (pi > 0.0 ? -acc / pi : 0.0);
        for (int s = 0; s < K; ++s) v += dpp[(size_t)s * N + i];
        dpa[i] = v;
    }
    __syncthreads();                                                        // every read of Cb_t+1 / Yb_t+1 by another thread is done
    for (int t = tid; t < NN; t += NT) {
        const int i = t / N, j = t - i * N;
        double v = c.fs ? mix_cbar(c, first, b, t) : 0.0;
        for (int s = 0; s < K; ++s) v += Ap[(size_t)s * NN + t];
        Cbar[t] = (pw(i) > 0.0 && pw(j) > 0.0) ? v : 0.0;
    }
    for (int t = tid; t < Nd; t += NT) {
        double v = c.ff ? mix_ybar(c, first, b, t) : 0.0;
        for (int s = 0; s < K; ++s) v += Ypt[(size_t)s * Nd + t];
        Ybar[t] = pw(t / d) > 0.0 ? v : 0.0;
    }
}

// every output rounded to fp32 once; dlambdas summed over the molecules, b ascending (by workgroup 0)
__global__ void __launch_bounds__(256) k_fgw_mixup_bwd_final(MixBwdCall c) {
    const int b = blockIdx.x, tid = threadIdx.x, NT = 256;
    const int N = c.N, d = c.d, NN = N * N, Nd = N * d, K = c.K, B = c.B;
    const bool ran = mix_outer(c, b) > 0, bad = mix_flagged(c, b);       // (no outer iteration: the starts are the outputs)
    const float nan = __builtin_nanf("");
    const double *Cbar = mix_at(c, c.w.Cbar) + (size_t)b * NN, *Ybar = mix_at(c, c.w.Ybar) + (size_t)b * Nd, *dpa = mix_at(c, c.w.dpacc) + (size_t)b * N;
    const double *dCa = mix_at(c, c.w.dCsacc) + (size_t)b * K * NN, *dYa = mix_at(c, c.w.dYsacc) + (size_t)b * K * Nd;
    const double *dpsa = mix_at(c, c.w.dpsacc) + (size_t)b * K * N;
    auto qw = [&](int s, int j) { return c.ps ? c.ps[((size_t)b * K + s) * N + j] : 1.f; };
    auto pw = [&](int i) { return c.p ? c.p[(size_t)b * N + i] : 1.f; };
    for (int t = tid; t < K * NN; t += NT) {
        const int s = t / NN, r = t - s * NN, i = r / N, j = r - i * N;
        if (c.dCs) c.dCs[(size_t)b * K * NN + t] = bad ? nan : (ran && qw(s, i) > 0.f && qw(s, j) > 0.f) ? (float)dCa[t] : 0.f;
    }
    for (int t = tid; t < K * Nd; t += NT) {
        const int s = t / Nd, j = (t - s * Nd) / d;
        if (c.dYs) c.dYs[(size_t)b * K * Nd + t] = bad ? nan : (ran && qw(s, j) > 0.f) ? (float)dYa[t] : 0.f;
    }
    for (int t = tid; t < K * N; t += NT) {
        const int s = t / N, j = t - s * N;
        if (c.dps) c.dps[(size_t)b * K * N + t] = bad ? nan : (ran && qw(s, j) > 0.f) ? (float)dpsa[t] : 0.f;
    }
    for (int i = tid; i < N; i += NT)
        if (c.dp) c.dp[(size_t)b * N + i] = bad ? nan : (ran && pw(i) > 0.f) ? (float)dpa[i] : 0.f;
    for (int t = tid; t < NN; t += NT)
        if (c.dinit_C) c.dinit_C[(size_t)b * NN + t] = bad ? nan : ran ? (float)Cbar[t] : (c.dC ? c.dC[(size_t)b * NN + t] : 0.f);
    for (int t = tid; t < Nd; t += NT)
        if (c.dinit_Y) c.dinit_Y[(size_t)b * Nd + t] = bad ? nan : ran ? (float)Ybar[t] : (c.dY ? c.dY[(size_t)b * Nd + t] : 0.f);
    if (b == 0 && c.dlambdas) {
        const double *dla = mix_at(c, c.w.dlamacc);
        for (int s = tid; s < K; s += NT) {
            double v = 0.0;
            for (int m = 0; m < B; ++m) v += mix_flagged(c, m) ? (double)nan : (mix_outer(c, m) > 0 ? dla[(size_t)m * K + s] : 0.0);
            c.dlambdas[s] = (float)v;
        }
    }
}

}  // namespace

extern "C" {

int conan_fgw_mixup_barycenter_bwd_lds_resident(int N) { return N > 0 && MixStore::resident(N) ? 1 : 0; }

long long conan_fgw_mixup_barycenter_bwd_workspace_bytes(int B, int K, int N, int d, int epoch) {
    return (long long)mix_workspace(B, K, N, d, epoch).total;
}

int conan_fgw_mixup_barycenter_bwd(const float *Ys, const float *Cs, const float *ps, const float *p, const float *lambdas, const float *init_Y, int B,
                                   int K, int N, int d, const conan_fgw_params *params, double rho, int epoch, double eps, const int *info,
                                   const void *record, const float *dY, const float *dC, float *dYs, float *dCs, float *dps, float *dp,
                                   float *dlambdas, float *dinit_C, float *dinit_Y, float *T_chk, int *epochs_chk, void *workspace, void *stream) {
    if (!Ys || !Cs || !params || !info || !record || !workspace || B <= 0 || K <= 0 || N <= 0 || d <= 0) return CONAN_E_BADARG;
    if (!dY && !dC) return CONAN_E_BADARG;
    if ((dps && !ps) || (dp && !p) || (dlambdas && !lambdas) || (dinit_Y && !init_Y)) return CONAN_E_BADARG;
    if (params->max_iter <= 0 || epoch <= 0 || !(rho > 0.0 && rho <= 1.79769313486231570815e308) || !(eps == eps)) return CONAN_E_BADARG;
    if (params->fixed_features && !init_Y) return CONAN_E_BADARG;
    if (params->loss_fun != 0 && params->loss_fun != 1) return CONAN_E_BADARG;
    if (!MixStore::supported(N)) return CONAN_E_UNSUPPORTED;
    const bool lds = MixStore::resident(N);
    const int max_iter = params->max_iter;
    MixBwdCall c{};
    c.Ys = Ys; c.Cs = Cs; c.ps = ps; c.p = p; c.lambdas = lambdas; c.info = info;
    c.Crec = static_cast<const double *>(record); c.Yrec = c.Crec + (size_t)(max_iter + 1) * B * N * N;
    c.dY = dY; c.dC = dC; c.dYs = dYs; c.dCs = dCs; c.dps = dps; c.dp = dp; c.dlambdas = dlambdas; c.dinit_C = dinit_C; c.dinit_Y = dinit_Y;
    c.Tchk = T_chk; c.epochs_chk = epochs_chk;
    c.B = B; c.K = K; c.N = N; c.d = d; c.P = pitch_of(N); c.epoch = epoch; c.max_iter = max_iter;
    c.kl = params->loss_fun != 0; c.fs = params->fixed_structure != 0; c.ff = params->fixed_features != 0; c.has_init_Y = init_Y != nullptr;
    c.alpha = (double)params->alpha; c.rho = rho; c.eps = eps;
    c.ws = static_cast<char *>(workspace); c.w = mix_workspace(B, K, N, d, epoch);
    hipStream_t st = as_stream(stream);
    const size_t bytes = MixStore::lds_bytes(N);
    for (int t = max_iter - 1; t >= 0; --t) {
        if (lds) launch_lds(k_fgw_mixup_bwd_coupling<true>, B * K, 64 * UNROLL_NW, bytes, st, c, t);
        else launch_lds(k_fgw_mixup_bwd_coupling<false>, B * K, 64 * UNROLL_NW, bytes, st, c, t);
        k_fgw_mixup_bwd_reduce<<<B, 256, 0, st>>>(c, t);
    }
    k_fgw_mixup_bwd_final<<<B, 256, 0, st>>>(c);
    CONAN_LAUNCH_CHECK();
    return CONAN_OK;
}

}  // extern "C"
