// The reference's gradient through the unrolled Bregman half-steps of the pairwise BAPG FGW solve for gfx950: the backward of conan_fgw_pair_fwd
// (fgw_pair.hip) with solver BAPG (the reference's fgw_bregman, bregman.py:170-279: plain differentiable torch), square or kl loss, to M, C1, C2,
// p, q and the start G0, from the cotangents of the returned plan and of fgw_dist.  B pairs per launch, one workgroup of UNROLL_NW wavefronts per
// pair (conan_fgw_bregman_bwd; DESIGN.md 3.3, "Pairwise FGW, BAPG: the unrolled gradient").
//
// With h = 2 C2 (square) or log(C2 + 1e-15) (kl), alpha' = 1 - alpha, a half-step with input plan T is
//     df = -2 alpha C1 T h^T + alpha' M                                   (symmetric)
//     df = -alpha (C1 T h^T + C1^T T h) + alpha' M                        (not symmetric)
//     X = exp(-df / eps),  E = T o X,  s = E 1 (rows) or E^T 1 (columns),  T' = diag(p / s) E  or  E diag(q / s)
// and an iteration is a row half-step followed by a column half-step.
//
// Two steps, for the iterations the forward ran (info[b,0], read here, clamped to [0, max_iter]; the stop decisions carry no gradient):
//
// (1) Replay, in fp64 from G0 or p q^T.  EVERY half-step's input plan goes to the pair's slice of the workspace (2 per iteration: the reverse
//     walk then re-forms nothing but X).  The final plan goes to T_chk, the iteration count and the flags to binfo.
// (2) Reverse walk.  Seed Gb = dT + ddist * d fgw_dist / dT at the final plan, accumulators seeded with ddist times the direct partials of
//     fgw_dist = alpha' sum M o T + alpha sum ((c0 1^T + 1 r0^T) - C1 T h^T) o T,  c0 = f1(C1) p,  r0 = f2(C2) q  (square: f1 = f2 = x^2; kl:
//     f1 = a log(a + 1e-15) - a, f2 = b).  Then for each half-step, last to first, with its recorded input T_k: X, s again; with l the line
//     (row or column) of an entry and m = p or q,
//         g_l = sum over the line of Gb o T'        dm_l += g_l / m_l        dE = Gb m_l / s_l - g_l / s_l        D = -dE o E / eps
//         dM += alpha' D                            Gb <- dE o X + (the products below)
//         symmetric:      dC1 -= 2 alpha D h T_k^T                 dh = -2 alpha D^T C1 T_k                    Gb -= 2 alpha C1^T D h
//         not symmetric:  dC1 -= alpha (D h T_k^T + T_k h D^T)     dh = -alpha (D^T C1 T_k + T_k^T C1 D)       Gb -= alpha (C1^T D h + C1 D h^T)
//         dC2 += h' o dh,  h' = 2 (square) or 1 / (C2 + 1e-15) (kl).
//     At the end dG0 = Gb, or without a start dp += Gb q, dq += Gb^T p.  No plan entry is ever a divisor or the argument of a logarithm: exact
//     zeros and denormals of a plan need nothing special.
//
// Products per half-step, all on fp64 MFMA (mm_f64_glb; mm_f64_pad where the LEFT operand is transposed): symmetric 2 to form X (C1 T_k, kept
// for D^T (C1 T_k), and (C1 T_k) h^T) in the replay, and in the walk the same 2 + 4 (D^T (C1 T_k), D h, (D h) T_k^T, C1^T (D h)): 8 against the
// forward's 2; not symmetric 4 in the replay and 4 + 9 in the walk.  Under kl h is formed once, in fp64, in the workspace (the forward takes the
// logarithm at every operand read).
//
// The conventions this kernel shares with its siblings (precisions, summation order, loop bounds, nodes without mass, NaN, storage) are
// stated once, in fgw_unroll.h, with the pieces the kernels can share.
//
// Nodes without mass (p_i = 0 or q_j = 0: how rectangular and own-size pairs are embedded): their entries of every T_k are exactly zero and
// their scaling factor is 0, so Gb and D are zero there, their rows / columns of dM, dC1, dC2, dG0 and their dp_i / dq_j are written as exactly
// 0.  A pair whose forward raised flags bit 2, or whose replay meets a zero (or NaN) sum on a node with mass or a non-finite plan entry, gets
// NaN in every gradient and binfo flag bit 2.
//
// Storage (fgw_unroll.h): the five matrices are T_k, X, Gb, D and a product buffer (conan_fgw_bregman_bwd_lds_resident: N <= 61).  The record,
// the three accumulators and h live in the workspace at every size.
#include "fgw_unroll.h"
#include "../../include/conan_fgw_hip_bregman_grad.h"

namespace {

struct BregmanBwdCall : UnrollPairIO {      // A = C1, B = C2, a = p, b = q, X0 = G0, dX = dT, chk = T_chk
    int *binfo;
    int N, P, max_iter, symmetric;
    double alpha, eps;                // (fp64 from the host: the scalar unit has no fp64 conversions)
    char *ws;
    size_t ws_stride;                 // bytes per pair
};

// vectors: p, q, the sums s, the scalings, g, dp, dq, c0, r0, two work lines (T 1 and T^T 1, the sums of the start) [N] each; no reduction space
using BregmanStore = UnrollStore<11, false>;
inline size_t bgb_stride(int N, int max_iter) { return BregmanStore::stride(N, ((size_t)2 * max_iter + 4) * N * N * 8); }      // the record, the three accumulators and h

// Registers (-Rpass-analysis=kernel-resource-usage): the second __launch_bounds__ argument, 4 = held at 128 VGPRs so that two
// workgroups share a CU, 2 = unbounded.  Unbounded the compiler takes 127 (LDS, square, symmetric), 129 - 138 (the other LDS-resident
// instantiations) and 131 - 149 (streamed) VGPRs with no scratch; held, 124 - 128 with at most 36 (LDS) / 64 (streamed) bytes of scratch per
// lane.  Measured on the backward launch alone (tools/probe_fgw_bregman_unrolled.py --ab-lib, B = 1280, N = 33 / B = 192, N = 90, 100
// iterations): LDS, kl, symmetric: held is 24 % faster (129 registers leave one workgroup per CU); LDS, square, symmetric: unbounded fits 128
// anyway and is 6 % faster than the held schedule; streamed: unbounded is 4 - 5 % faster.  So: held where LDS-resident and (kl or not
// symmetric), unbounded elsewhere; the two LDS-resident not-symmetric instantiations follow the kl one's register count, not a timing of
// their own.  -DCONAN_BREGMAN_BWD_AB=1 builds the opposite choice everywhere, for that A/B.
#ifndef CONAN_BREGMAN_BWD_AB
#define CONAN_BREGMAN_BWD_AB 0
#endif
constexpr int bgb_min_blocks(bool lds, bool kl, bool asym) { return ((lds && (kl || asym)) != (CONAN_BREGMAN_BWD_AB != 0)) ? 4 : 2; }
template <bool LDS, bool KL, bool ASYM>
__global__ void __launch_bounds__(64 * UNROLL_NW, bgb_min_blocks(LDS, KL, ASYM)) k_fgw_bregman_bwd(BregmanBwdCall c) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int NW = UNROLL_NW, NT = 64 * NW;
    using h_t = std::conditional_t<KL, double, float>;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int N = c.N, P = c.P, NN = N * N;
    double *pa = reinterpret_cast<double *>(smem), *qb = pa + N, *sv = qb + N, *sc = sv + N, *gv = sc + N, *dpa = gv + N, *dqa = dpa + N;
    double *c0 = dqa + N, *r0 = c0 + N, *zc = r0 + N, *wc = zc + N;
    double *pm = wc + N;
    double *rec = reinterpret_cast<double *>(c.ws + (size_t)b * c.ws_stride);                  // the input plan of half-step 0 .. 2 max_iter - 1, [N,N] each
    double *dMa = rec + (size_t)2 * c.max_iter * NN, *dC1a = dMa + NN, *dC2a = dC1a + NN, *hm = dC2a + NN;
    double *Tk = LDS ? reinterpret_cast<double *>(smem + BregmanStore::vec_bytes(N)) : hm + NN;
    double *Xb = Tk + N * P, *Gb = Xb + N * P, *D = Gb + N * P, *A = D + N * P;
    const float *Mg = c.M + (size_t)b * NN, *C1g = c.A + (size_t)b * NN, *C2g = c.B + (size_t)b * NN;
    const float *G0g = c.X0 ? c.X0 + (size_t)b * NN : nullptr, *dTg = c.dX ? c.dX + (size_t)b * NN : nullptr;
    const double alpha = c.alpha, om = 1.0 - alpha, eps = c.eps;
    constexpr double hs = KL ? 1.0 : 2.0;                                                       // h = hs * (the matrix the products read)
    const double ah = alpha * hs;
    const int iters = __builtin_amdgcn_readfirstlane(min(max(c.info[b * 4 + 0], 0), c.max_iter));      // a corrupt info can neither leave the record nor lengthen a loop
    const int fwd_flags = __builtin_amdgcn_readfirstlane(c.info[b * 4 + 2]);
    bool asym = false;
    if constexpr (ASYM) asym = c.symmetric < 0 ? __builtin_amdgcn_readfirstlane(c.info[b * 4 + 3]) == 0 : true;
    const h_t *hg;                                                                              // kl: log(C2 + 1e-15) in fp64; square: C2 itself
    if constexpr (KL) hg = hm; else hg = C2g;

    auto line_sums = [&](bool col, auto f, double *out) { unroll_line_sums(tid, lane, wave, N, P, pm, col, f, out); };
    auto live = [&](int i, int j) { return unroll_live(pa, qb, i, j); };
    // X h (WT = false) or X h^T (WT = true) without the factor hs; X [N,N] at pitch P
    auto mm_h = [&](auto wt, const double *X, auto st) { mm_f64_glb<NW, decltype(wt)::value>(N, N, N, X, P, hg, N, st); };
    auto f1 = [&](double a) { return KL ? a * log(a + 1e-15) - a : a * a; };
    auto f1d = [&](double a) { return KL ? log(a + 1e-15) + a / (a + 1e-15) - 1.0 : 2.0 * a; };
    auto f2 = [&](double e) { return KL ? e : e * e; };
    auto f2d = [&](double e) { return KL ? 1.0 : 2.0 * e; };
    auto hd = [&](double e) { return KL ? 1.0 / (e + 1e-15) : 2.0; };

    for (int i = tid; i < N; i += NT) {
        pa[i] = c.a ? (double)c.a[(size_t)b * N + i] : 1.0 / (double)N;
        qb[i] = c.b ? (double)c.b[(size_t)b * N + i] : 1.0 / (double)N;
        dpa[i] = 0.0; dqa[i] = 0.0;
    }
    if constexpr (KL)
        for (int t = tid; t < NN; t += NT) hm[t] = log((double)C2g[t] + 1e-15);
    __syncthreads();
    for (int i = tid; i < N; i += NT) {                                     // the untransposed init_matrix (fgw_dist's, in every case)
        double s1 = 0.0, s2 = 0.0;
        for (int k = 0; k < N; ++k) { s1 += f1((double)C1g[i * N + k]) * pa[k]; s2 += f2((double)C2g[i * N + k]) * qb[k]; }
        c0[i] = s1; r0[i] = s2;
    }
    __syncthreads();                                                        // (hm is read by the whole workgroup from here on)

    int bad = 0;                                                            // per thread: a zero sum on a node with mass, or a non-finite plan entry

    // The half-step with input plan Tk: X (zero at entries without mass) to Xb, the line sums of Tk o X to sv, mass / sum to sc; leaves
    // A = C1 Tk (symmetric) or C1^T Tk.  Uses D as a product buffer when not symmetric.  Ends on a barrier.
    auto half = [&](bool col) {
        auto xf = [&](int i, int j, double g) { return live(i, j) ? exp((g - om * (double)Mg[i * N + j]) / eps) : 0.0; };      // g: the product terms with their factor
        mm_f64_glb<NW, false>(N, N, N, C1g, N, Tk, P, [&](int i, int j, double v) { A[i * P + j] = v; });              // C1 Tk
        __syncthreads();
        bool done = false;
        if constexpr (ASYM) {
            if (asym) {
                mm_h(std::true_type{}, A, [&](int i, int j, double g) { D[i * P + j] = g; });                            // C1 Tk h^T
                __syncthreads();
                mm_f64_pad<NW>(N, N, N, [&](int i, int k) { return (double)C1g[k * N + i]; }, [&](int k, int j) { return Tk[k * P + j]; },
                               [&](int i, int j, double v) { A[i * P + j] = v; });                                      // C1^T Tk
                __syncthreads();
                mm_h(std::false_type{}, A, [&](int i, int j, double g) { Xb[i * P + j] = xf(i, j, ah * (D[i * P + j] + g)); });
                done = true;
            }
        }
        if (!done) mm_h(std::true_type{}, A, [&](int i, int j, double g) { Xb[i * P + j] = xf(i, j, 2.0 * ah * g); });
        __syncthreads();
        line_sums(col, [&](int, int, int o) { return Tk[o] * Xb[o]; }, sv);
        for (int l = tid; l < N; l += NT) {
            const double m = col ? qb[l] : pa[l], s = sv[l];
            if (m > 0.0 && !(s > 0.0)) bad = 1;                             // m / 0: the reference's NaN (inf * 0) follows
            sc[l] = m > 0.0 ? m / s : 0.0;
        }
        __syncthreads();
    };

    // ---- step 1: the forward's half-steps again in fp64, every input plan to the record ----------------------------------------------------------
    for (int t = tid; t < NN; t += NT) {
        const int i = t / N, j = t - i * N;
        const double x0 = G0g ? (double)G0g[t] : pa[i] * qb[j];
        Tk[i * P + j] = live(i, j) ? x0 : 0.0;
    }
    __syncthreads();
    for (int k = 0; k < 2 * iters; ++k) {
        const bool col = (k & 1) != 0;
        double *r = rec + (size_t)k * NN;
        for (int t = tid; t < NN; t += NT) { const int i = t / N, j = t - i * N; r[t] = Tk[i * P + j]; }
        half(col);
        for (int t = tid; t < NN; t += NT) {
            const int i = t / N, j = t - i * N, o = i * P + j;
            const double v = Tk[o] * Xb[o] * sc[col ? j : i];
            if (!(fabs(v) < __builtin_inf())) bad = 1;
            Tk[o] = v;
        }
        __syncthreads();
    }
    if (c.chk)
        for (int t = tid; t < NN; t += NT) { const int i = t / N, j = t - i * N; c.chk[(size_t)b * NN + t] = (float)Tk[i * P + j]; }
    const bool flagged = __syncthreads_or(bad) != 0 || (fwd_flags & 4) != 0;                                            // (workgroup-uniform)
    if (c.binfo && tid == 0) {
        c.binfo[b * 2 + 0] = iters;
        c.binfo[b * 2 + 1] = flagged ? 4 : 0;
    }
    if (flagged) {                                                          // the reference's autograd gives NaN: so do we, everywhere
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

    // ---- step 2a: the cotangent of the final plan and the direct partials of fgw_dist (Tk holds the final plan) ----------------------------------
    if (c.ddist) {                                                          // (workgroup-uniform)
        const double dd = (double)c.ddist[b], da = dd * alpha;
        line_sums(false, [&](int, int, int o) { return Tk[o]; }, zc);      // T 1
        line_sums(true, [&](int, int, int o) { return Tk[o]; }, wc);       // T^T 1
        for (int l = tid; l < N; l += NT) {
            double s1 = 0.0, s2 = 0.0;
            for (int i = 0; i < N; ++i) { s1 += f1((double)C1g[i * N + l]) * zc[i]; s2 += f2((double)C2g[i * N + l]) * wc[i]; }
            dpa[l] = da * s1; dqa[l] = da * s2;
        }
        mm_f64_glb<NW, false>(N, N, N, C1g, N, Tk, P, [&](int i, int j, double v) { A[i * P + j] = v; });              // C1 T
        for (int t = tid; t < NN; t += NT) { const int i = t / N, j = t - i * N; dMa[t] = dd * om * Tk[i * P + j]; }
        __syncthreads();
        mm_h(std::true_type{}, A, [&](int i, int j, double g) {                                                          // C1 T h^T
            const double dx = dTg ? (double)dTg[i * N + j] : 0.0;
            Gb[i * P + j] = dx + dd * (om * (double)Mg[i * N + j] + alpha * (c0[i] + r0[j]) - ah * g);
        });
        mm_f64_pad<NW>(N, N, N, [&](int j, int k) { return Tk[k * P + j]; }, [&](int k, int l) { return A[k * P + l]; }, [&](int j, int l, double v) {
            const double e = (double)C2g[j * N + l];
            dC2a[j * N + l] = da * (f2d(e) * wc[j] * qb[l] - hd(e) * v);                                                // T^T C1 T
        });
        __syncthreads();
        mm_h(std::false_type{}, Tk, [&](int i, int j, double v) { A[i * P + j] = v; });                                 // T h
        __syncthreads();
        mm_f64_glb<NW, true>(N, N, N, A, P, Tk, P, [&](int i, int l, double v) {
            dC1a[i * N + l] = da * (f1d((double)C1g[i * N + l]) * zc[i] * pa[l] - hs * v);                              // T h T^T
        });
        mm_f64_pad<NW>(N, N, N, [&](int i, int k) { return (double)C1g[k * N + i]; }, [&](int k, int j) { return A[k * P + j]; }, [&](int i, int j, double v) {
            Gb[i * P + j] = live(i, j) ? Gb[i * P + j] - dd * ah * v : 0.0;                                              // C1^T T h
        });
    } else {
        for (int t = tid; t < NN; t += NT) {
            const int i = t / N, j = t - i * N;
            Gb[i * P + j] = live(i, j) ? (double)dTg[t] : 0.0;
            dMa[t] = 0.0; dC1a[t] = 0.0; dC2a[t] = 0.0;
        }
    }
    __syncthreads();

    // ---- step 2b: the half-steps in reverse ------------------------------------------------------------------------------------------------------
    for (int k = 2 * iters - 1; k >= 0; --k) {
        const bool col = (k & 1) != 0;
        const double *xr = rec + (size_t)k * NN;
        for (int t = tid; t < NN; t += NT) { const int i = t / N, j = t - i * N; Tk[i * P + j] = xr[t]; }
        __syncthreads();
        half(col);                                                          // A = C1 Tk (symmetric) or C1^T Tk
        line_sums(col, [&](int l, int, int o) { return Gb[o] * (Tk[o] * Xb[o] * sc[l]); }, gv);
        for (int l = tid; l < N; l += NT) {
            if (col) { if (qb[l] > 0.0) dqa[l] += gv[l] / qb[l]; }
            else if (pa[l] > 0.0) dpa[l] += gv[l] / pa[l];
        }
        for (int t = tid; t < NN; t += NT) {
            const int i = t / N, j = t - i * N, o = i * P + j, l = col ? j : i;
            double dE = 0.0;
            if (live(i, j)) dE = Gb[o] * sc[l] - gv[l] / sv[l];
            const double x = Xb[o], d = -dE * (Tk[o] * x) / eps;
            D[o] = d; Gb[o] = dE * x;
            dMa[t] += om * d;
        }
        __syncthreads();
        bool done = false;
        if constexpr (ASYM) {
            if (asym) {
                mm_f64_pad<NW>(N, N, N, [&](int j, int kk) { return A[kk * P + j]; }, [&](int kk, int l) { return D[kk * P + l]; }, [&](int j, int l, double v) {
                    dC2a[j * N + l] -= alpha * hd((double)C2g[j * N + l]) * v;                                          // Tk^T C1 D
                });
                __syncthreads();
                mm_f64_glb<NW, false>(N, N, N, C1g, N, Tk, P, [&](int i, int j, double v) { A[i * P + j] = v; });      // C1 Tk
                __syncthreads();
                mm_f64_pad<NW>(N, N, N, [&](int j, int kk) { return D[kk * P + j]; }, [&](int kk, int l) { return A[kk * P + l]; }, [&](int j, int l, double v) {
                    dC2a[j * N + l] -= alpha * hd((double)C2g[j * N + l]) * v;                                          // D^T C1 Tk
                });
                __syncthreads();
                mm_h(std::false_type{}, D, [&](int i, int j, double v) { A[i * P + j] = v; });                          // D h
                __syncthreads();
                mm_f64_glb<NW, true>(N, N, N, A, P, Tk, P, [&](int i, int l, double v) { dC1a[i * N + l] -= ah * v; });             // D h Tk^T
                mm_f64_pad<NW>(N, N, N, [&](int i, int kk) { return (double)C1g[kk * N + i]; }, [&](int kk, int j) { return A[kk * P + j]; },
                               [&](int i, int j, double v) { Gb[i * P + j] -= ah * v; });                               // C1^T D h
                __syncthreads();
                mm_h(std::true_type{}, D, [&](int i, int j, double v) { A[i * P + j] = v; });                           // D h^T
                __syncthreads();
                mm_f64_glb<NW, true>(N, N, N, Tk, P, A, P, [&](int i, int l, double v) { dC1a[i * N + l] -= ah * v; });             // Tk h D^T
                mm_f64_glb<NW, false>(N, N, N, C1g, N, A, P, [&](int i, int j, double v) {
                    Gb[i * P + j] = live(i, j) ? Gb[i * P + j] - ah * v : 0.0;                                           // C1 D h^T
                });
                done = true;
            }
        }
        if (!done) {
            mm_f64_pad<NW>(N, N, N, [&](int j, int kk) { return D[kk * P + j]; }, [&](int kk, int l) { return A[kk * P + l]; }, [&](int j, int l, double v) {
                dC2a[j * N + l] -= 2.0 * alpha * hd((double)C2g[j * N + l]) * v;                                        // D^T (C1 Tk)
            });
            __syncthreads();
            mm_h(std::false_type{}, D, [&](int i, int j, double v) { A[i * P + j] = v; });                              // D h
            __syncthreads();
            mm_f64_glb<NW, true>(N, N, N, A, P, Tk, P, [&](int i, int l, double v) { dC1a[i * N + l] -= 2.0 * ah * v; });           // D h Tk^T
            mm_f64_pad<NW>(N, N, N, [&](int i, int kk) { return (double)C1g[kk * N + i]; }, [&](int kk, int j) { return A[kk * P + j]; }, [&](int i, int j, double v) {
                Gb[i * P + j] = live(i, j) ? Gb[i * P + j] - 2.0 * ah * v : 0.0;                                         // C1^T D h
            });
        }
        __syncthreads();
    }

    // ---- the start: its own gradient, or through p q^T to the weights -----------------------------------------------------------------------------
    if (!G0g) {
        unroll_start_sums(tid, lane, wave, N, P, pm, Gb, pa, qb, zc, wc);
        for (int i = tid; i < N; i += NT) { dpa[i] += zc[i]; dqa[i] += wc[i]; }
        __syncthreads();
    }
    for (int t = tid; t < NN; t += NT) {
        const int i = t / N, j = t - i * N;
        c.dM[(size_t)b * NN + t] = live(i, j) ? (float)dMa[t] : 0.f;
        c.dA[(size_t)b * NN + t] = (pa[i] > 0.0 && pa[j] > 0.0) ? (float)dC1a[t] : 0.f;
        c.dB[(size_t)b * NN + t] = (qb[i] > 0.0 && qb[j] > 0.0) ? (float)dC2a[t] : 0.f;
        if (c.dX0) c.dX0[(size_t)b * NN + t] = live(i, j) ? (float)Gb[i * P + j] : 0.f;
    }
    for (int i = tid; i < N; i += NT) {
        if (c.da) c.da[(size_t)b * N + i] = pa[i] > 0.0 ? (float)dpa[i] : 0.f;
        if (c.db) c.db[(size_t)b * N + i] = qb[i] > 0.0 ? (float)dqa[i] : 0.f;
    }
}

}  // namespace

extern "C" {

int conan_fgw_bregman_bwd_lds_resident(int N) { return N > 0 && BregmanStore::resident(N) ? 1 : 0; }

long long conan_fgw_bregman_bwd_workspace_bytes(int B, int N, int max_iter) {
    if (B <= 0 || max_iter <= 0 || !BregmanStore::supported(N)) return 0;
    return (long long)((size_t)B * bgb_stride(N, max_iter));
}

int conan_fgw_bregman_bwd(const float *M, const float *C1, const float *C2, const float *p, const float *q, const float *G0, int B, int N, double alpha,
                          double epsilon, int max_iter, int loss_fun, int symmetric, const int *info, const float *dT, const float *ddist, float *dM,
                          float *dC1, float *dC2, float *dp, float *dq, float *dG0, float *T_chk, int *binfo, void *workspace, void *stream) {
    BregmanBwdCall c{};
    static_cast<UnrollPairIO &>(c) = {M, C1, C2, p, q, G0, info, dT, ddist, dM, dC1, dC2, dp, dq, dG0, T_chk};
    if (max_iter <= 0 || unroll_pair_args(c, B, N, workspace, epsilon, alpha) != CONAN_OK) return CONAN_E_BADARG;
    if (loss_fun < 0 || loss_fun > 1 || symmetric < -1 || symmetric > 1) return CONAN_E_BADARG;
    if (!BregmanStore::supported(N)) return CONAN_E_UNSUPPORTED;
    c.binfo = binfo;
    c.N = N; c.P = pitch_of(N); c.max_iter = max_iter; c.symmetric = symmetric;
    c.alpha = alpha; c.eps = epsilon;
    c.ws = static_cast<char *>(workspace); c.ws_stride = bgb_stride(N, max_iter);
    with_flags([&](auto L, auto K, auto A) {
        launch_lds(k_fgw_bregman_bwd<decltype(L)::value, decltype(K)::value, decltype(A)::value>, B, 64 * UNROLL_NW, BregmanStore::lds_bytes(N), as_stream(stream), c);
    }, BregmanStore::resident(N), loss_fun == 1, symmetric != 1);
    CONAN_LAUNCH_CHECK();
    return CONAN_OK;
}

}  // extern "C"
