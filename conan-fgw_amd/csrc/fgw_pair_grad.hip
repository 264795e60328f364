// The reference's gradient through the unrolled iterations of the pairwise entropic FGW solve for gfx950: the backward of conan_fgw_pair_fwd
// (fgw_pair.hip) with solver PGD or PPA and the square loss (the reference's fgw_projected, bregman.py:70-167, around sinkhorn_log,
// sinkhorn.py:388-450: plain differentiable torch) to M, C1, C2, p, q and the start G0, from the cotangents of the returned plan and of fgw_dist.
// B pairs per launch, one workgroup of UNROLL_NW wavefronts per pair (conan_fgw_pair_bwd; DESIGN.md 3.3, "Pairwise FGW: the unrolled gradient").
//
// With c_i = sum_l C1_il^2 p_l, r_j = sum_l C2_jl^2 q_l (c', r': the same of the transposes), alpha' = 1 - alpha, an outer iteration is
//     tens = 2 alpha (c 1^T + 1 r^T) - 4 alpha C1 T_k C2^T + alpha' M                                                       (symmetric)
//     tens = alpha ((c + c') 1^T + 1 (r + r')^T) - 2 alpha (C1 T_k C2^T + C1^T T_k C2) + alpha' M                           (not symmetric)
//     PPA: tens -= eps log T_k;      Mr = -tens / eps;      T_(k+1) = diag(u^S) K diag(v^S),  K = exp(Mr - column maximum),
//     u^0 = 1,  v^t = q / (K^T u^(t-1)),  u^t = p / (K v^t),  t = 1 .. S_k        (sinkhorn_log from zero potentials, in its scaling form).
//
// Two steps, for the outer iterations the forward ran (info[b,0], read here, clamped to [0, max_iter]):
//
// (1) Replay, in fp64 from G0 or p q^T.  Every iteration's input plan T_k goes to the pair's slice of the workspace, with the sweeps S_k its
//     Sinkhorn call ran: decided here by the reference's rule (the marginal error ||v o (K^T u) - q|| evaluated where ii % 10 == 0, exit below
//     stop_thr, at most num_iter_max), because the forward reports only their sum.  The stop decisions carry no gradient.  The final plan goes
//     to T_chk, the sweep total and the flags to binfo.
// (2) Reverse walk.  Seed Gb = dT + ddist * d fgw_dist / dT at the final plan, accumulators seeded with ddist times the direct partials of
//     fgw_dist (conan_fgw_pair_dist_bwd's formulas, formed here in fp64).  Then for k = last .. 0: K and the S_k sweeps again with every u^t, v^t
//     kept; the Sinkhorn reverse sweeps with plan cotangent Gb (sinkhorn_grad.hip's recurrences: fb_i = sum_j Gb_ij T_ij, gb likewise, then
//     z = fb o u^t / p, la += fb, gb -= v^t o (K^T z), w = gb o v^t / q, lb += gb, fb = -u^(t-1) o (K w), gb = 0 for t = S .. 1); ONE product over
//     the kept factors, [z^1.. | u^0..] [v^1.. | w^1..]^T on fp64 MFMA, gives D = d tens = -(Gb o T - K o product) / eps; dp += la / p,
//     dq += lb / q; and with rho = D 1, kappa = D^T 1 (symmetric):
//         dM += alpha' D            dC1 += 4 alpha (C1 o rho p^T) - 4 alpha D C2 T_k^T        dp_l += 2 alpha sum_i C1_il^2 rho_i
//         Gb <- -4 alpha C1^T D C2   dC2 += 4 alpha (C2 o kappa q^T) - 4 alpha D^T C1 T_k      dq_l += 2 alpha sum_j C2_jl^2 kappa_j
//     (not symmetric: the average of these and their transposed twins; PPA: Gb -= eps D / T_k).  At the end dG0 = Gb, or without a start
//     dp += Gb q, dq += Gb^T p.
//
// Products per outer iteration, all on fp64 MFMA (mm_f64_glb; mm_f64_pad where the LEFT operand is transposed): symmetric 2 to form tens
// (C1 T_k, which is kept for D^T (C1 T_k), and (C1 T_k) C2^T) + the factor product + 4 = 7 of size N^3 (the factor product is N^2 * 2 S_k);
// not symmetric 4 + 1 + 9.  Each Sinkhorn sweep is two matrix-vector passes forward and two in reverse.
//
// The conventions this kernel shares with its siblings (precisions, summation order, loop bounds, nodes without mass, NaN, storage) are
// stated once, in fgw_unroll.h, with the pieces the kernels can share.
//
// Nodes without mass (p_i = 0 or q_j = 0: how rectangular and own-size pairs are embedded): their entries of K and of every T_k are exactly
// zero and constants of the solve, so Gb and D are zero there, their rows / columns of dM, dC1, dC2, dG0 and their dp_i / dq_j are written as
// exactly 0 (the documented deviation of the sibling kernels).  A pair whose forward raised flags bit 2, or whose replay meets a non-finite plan
// entry or, under PPA, an exact zero of an input plan at an entry with mass (log 0: the reference's NaN), gets NaN in every gradient and binfo
// flag bit 2.
//
// Storage (fgw_unroll.h): the five matrices are T_k, K, Gb, D and a product buffer (conan_fgw_pair_bwd_lds_resident: N <= 61).  The record, the
// three accumulators and the Sinkhorn factors of the current iteration live in the workspace at every size.
#include "fgw_unroll.h"
#include "../../include/conan_fgw_hip_pair_grad.h"

namespace {

struct PairBwdCall : UnrollPairIO {   // A = C1, B = C2, a = p, b = q, X0 = G0, dX = dT, chk = T_chk
    int *binfo;
    int N, P, max_iter, num_iter_max, ppa, symmetric;
    double alpha, eps, stop_thr;      // (fp64 from the host: the scalar unit has no fp64 conversions)
    char *ws;
    size_t ws_stride;                 // bytes per pair
};

// vectors: p, q, u, v, fb, gb, la, lb, z, w, dp, dq, the row / column constants of tens and of fgw_dist [N] each, and reduction space
using PairStore = UnrollStore<16, true>;
__host__ __device__ inline size_t pgb_srec_bytes(int max_iter) { return (size_t)((max_iter + 1) / 2) * 8; }
inline size_t pgb_stride(int N, int max_iter, int nim) {      // the record, the three accumulators, the Sinkhorn factors and the sweep counts
    return PairStore::stride(N, ((size_t)max_iter + 3) * N * N * 8 + ((size_t)4 * nim + 2) * N * 8 + pgb_srec_bytes(max_iter));
}

// Registers: unbounded the compiler takes 177 (LDS) / 183 (streamed) VGPRs, one workgroup of 8 wavefronts per CU; held at 128 it spills 232 / 212
// bytes of scratch per lane and two workgroups share a CU.  Measured on the backward alone: at N = 33, B = 1280 the spilling
// build is 1.33 - 1.49 times faster (more workgroups than CUs: the second one hides the first one's barriers and LDS round trips); at
// N = 90, B = 192 it is 2 - 7 % slower.  So the LDS-resident kernel is held at 128 and the streamed one is not.
template <bool LDS>
__global__ void __launch_bounds__(64 * UNROLL_NW, LDS ? 4 : 2) k_fgw_pair_bwd(PairBwdCall c) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int NW = UNROLL_NW, NT = 64 * NW;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int N = c.N, P = c.P, NN = N * N, nim = c.num_iter_max;
    double *pa = reinterpret_cast<double *>(smem), *qb = pa + N, *uc = qb + N, *vc = uc + N, *fb = vc + N, *gb = fb + N, *la = gb + N, *lb = la + N;
    double *zc = lb + N, *wc = zc + N, *dpa = wc + N, *dqa = dpa + N, *cr = dqa + N, *cc = cr + N, *c0 = cc + N, *r0 = c0 + N;
    double *red = r0 + N, *pm = red + 16;
    double *rec = reinterpret_cast<double *>(c.ws + (size_t)b * c.ws_stride);                  // T_0 .. T_(max_iter - 1) [N,N] each
    double *dMa = rec + (size_t)c.max_iter * NN, *dC1a = dMa + NN, *dC2a = dC1a + NN;
    double *hU = dC2a + NN;                                                                     // u^0 .. u^nim [nim + 1][N]
    double *hV = hU + (size_t)(nim + 1) * N;                                                    // v^0 .. v^nim (v^0 is never read)
    double *hZ = hV + (size_t)(nim + 1) * N;                                                    // z^1 .. z^nim [nim][N]
    double *hW = hZ + (size_t)nim * N;                                                          // w^1 .. w^nim
    int *srec = reinterpret_cast<int *>(hW + (size_t)nim * N);                                  // S_0 .. S_(max_iter - 1)
    double *Tk = LDS ? reinterpret_cast<double *>(smem + PairStore::vec_bytes(N)) : reinterpret_cast<double *>(reinterpret_cast<char *>(srec) + pgb_srec_bytes(c.max_iter));
    double *K = Tk + N * P, *Gb = K + N * P, *D = Gb + N * P, *A = D + N * P;
    const float *Mg = c.M + (size_t)b * NN, *C1g = c.A + (size_t)b * NN, *C2g = c.B + (size_t)b * NN;
    const float *G0g = c.X0 ? c.X0 + (size_t)b * NN : nullptr, *dTg = c.dX ? c.dX + (size_t)b * NN : nullptr;
    const double alpha = c.alpha, om = 1.0 - alpha, four_alpha = 4.0 * alpha, two_alpha = 2.0 * alpha, eps = c.eps;
    const bool ppa = c.ppa != 0;
    const int iters = __builtin_amdgcn_readfirstlane(min(max(c.info[b * 4 + 0], 0), c.max_iter));      // a corrupt info can neither leave the record nor lengthen a loop
    const int fwd_flags = __builtin_amdgcn_readfirstlane(c.info[b * 4 + 2]);
    const bool sym = c.symmetric < 0 ? __builtin_amdgcn_readfirstlane(c.info[b * 4 + 3]) != 0 : c.symmetric == 1;
    const double ninf = -__builtin_inf();

    auto line_sums = [&](bool col, auto f, double *out) { unroll_line_sums(tid, lane, wave, N, P, pm, col, f, out); };
    auto live = [&](int i, int j) { return unroll_live(pa, qb, i, j); };
    for (int i = tid; i < N; i += NT) {
        pa[i] = c.a ? (double)c.a[(size_t)b * N + i] : 1.0 / (double)N;
        qb[i] = c.b ? (double)c.b[(size_t)b * N + i] : 1.0 / (double)N;
        dpa[i] = 0.0; dqa[i] = 0.0;
    }
    __syncthreads();
    for (int i = tid; i < N; i += NT) {                                     // init_matrix of the problem and of its transpose
        double s1 = 0.0, s1t = 0.0, s2 = 0.0, s2t = 0.0;
        for (int k = 0; k < N; ++k) {
            const double a = (double)C1g[i * N + k], at = (double)C1g[k * N + i], e = (double)C2g[i * N + k], et = (double)C2g[k * N + i];
            s1 += a * a * pa[k]; s1t += at * at * pa[k];
            s2 += e * e * qb[k]; s2t += et * et * qb[k];
        }
        c0[i] = s1; r0[i] = s2;
        cr[i] = sym ? two_alpha * s1 : alpha * (s1 + s1t);
        cc[i] = sym ? two_alpha * s2 : alpha * (s2 + s2t);
    }
    __syncthreads();

    int bad = 0;                                                            // per thread: a non-finite plan entry, or PPA's log of an exact zero at an entry with mass

    // K = exp(Mr - column maximum) of the plan in Tk (zero at entries without mass); leaves A = C1 Tk (symmetric) or C1^T Tk.  Ends on a barrier.
    auto form_K = [&]() {
        auto mr = [&](int i, int j, double g) -> double {                  // g: the product term of tens with its factor
            if (!live(i, j)) return ninf;
            double tens = cr[i] + cc[j] - g + om * (double)Mg[i * N + j];
            if (ppa) {
                const double t = Tk[i * P + j];
                if (!(t > 0.0)) { bad = 1; return ninf; }
                tens -= eps * log(t);
            }
            return -tens / eps;
        };
        mm_f64_glb<NW, false>(N, N, N, C1g, N, Tk, P, [&](int i, int j, double v) { A[i * P + j] = v; });
        __syncthreads();
        if (sym) {
            mm_f64_glb<NW, true>(N, N, N, A, P, C2g, N, [&](int i, int j, double g) { K[i * P + j] = mr(i, j, four_alpha * g); });
        } else {
            mm_f64_glb<NW, true>(N, N, N, A, P, C2g, N, [&](int i, int j, double g) { K[i * P + j] = g; });           // C1 Tk C2^T
            __syncthreads();
            mm_f64_pad<NW>(N, N, N, [&](int i, int k) { return (double)C1g[k * N + i]; }, [&](int k, int j) { return Tk[k * P + j]; },
                           [&](int i, int j, double v) { A[i * P + j] = v; });                                          // C1^T Tk
            __syncthreads();
            mm_f64_glb<NW, false>(N, N, N, A, P, C2g, N, [&](int i, int j, double g) { K[i * P + j] = mr(i, j, two_alpha * (K[i * P + j] + g)); });
        }
        __syncthreads();
        for (int l = lane; l < N; l += 64) {                                // column maxima
            double m = ninf;
            for (int e = wave; e < N; e += NW) m = fmax(m, K[e * P + l]);
            pm[wave * N + l] = m;
        }
        __syncthreads();
        for (int l = tid; l < N; l += NT) {
            double m = pm[l];
#pragma unroll
            for (int u = 1; u < NW; ++u) m = fmax(m, pm[u * N + l]);
            wc[l] = m > ninf ? m : 0.0;
        }
        __syncthreads();
        for (int t = tid; t < NN; t += NT) {
            const int i = t / N, j = t - i * N;
            const double m = K[i * P + j];
            K[i * P + j] = m > ninf ? exp(m - wc[j]) : 0.0;
        }
        __syncthreads();
    };

    // sinkhorn_log's sweeps on K from zero potentials -> the sweeps run; u^S, v^S in uc, vc.  decide: the reference's exit rule, at most nim;
    // else exactly `fixed`.  keep: every u^t, v^t to hU, hV.  Every value that steers the loop comes out of block_sum_d: workgroup-uniform.
    auto sweeps = [&](bool decide, int fixed, bool keep) -> int {
        for (int i = tid; i < N; i += NT) {
            const double u0 = pa[i] > 0.0 ? 1.0 : 0.0;
            uc[i] = u0;
            if (keep) hU[i] = u0;
        }
        __syncthreads();
        const int lim = decide ? nim : fixed;
        int S = lim;
        for (int ii = 0; ii < lim; ++ii) {
            line_sums(true, [&](int, int e, int o) { return K[o] * uc[e]; }, vc);
            for (int j = tid; j < N; j += NT) {
                const double v = qb[j] > 0.0 ? qb[j] / vc[j] : 0.0;
                vc[j] = v;
                if (keep) hV[(size_t)(ii + 1) * N + j] = v;
            }
            __syncthreads();
            line_sums(false, [&](int, int e, int o) { return K[o] * vc[e]; }, uc);
            for (int i = tid; i < N; i += NT) {
                const double u = pa[i] > 0.0 ? pa[i] / uc[i] : 0.0;
                uc[i] = u;
                if (keep) hU[(size_t)(ii + 1) * N + i] = u;
            }
            __syncthreads();
            if (decide && ii % 10 == 0) {                                   // the marginal violation, sinkhorn.py:418-433
                line_sums(true, [&](int, int e, int o) { return K[o] * uc[e]; }, gb);
                double e2 = 0.0;
                for (int j = tid; j < N; j += NT) { const double df = vc[j] * gb[j] - qb[j]; e2 += df * df; }
                if (sqrt(block_sum_d<NW>(e2, red)) < c.stop_thr) { S = ii + 1; break; }
            }
        }
        return S;
    };

    // ---- step 1: the forward's iterations again in fp64, every input plan and its sweep count to the record ------------------------------------
    for (int t = tid; t < NN; t += NT) {
        const int i = t / N, j = t - i * N;
        const double x0 = G0g ? (double)G0g[t] : pa[i] * qb[j];
        Tk[i * P + j] = live(i, j) ? x0 : 0.0;
    }
    __syncthreads();
    int sk_total = 0;
    for (int k = 0; k < iters; ++k) {
        double *r = rec + (size_t)k * NN;
        for (int t = tid; t < NN; t += NT) { const int i = t / N, j = t - i * N; r[t] = Tk[i * P + j]; }
        form_K();
        const int S = sweeps(true, 0, false);
        if (tid == 0) srec[k] = S;
        sk_total += S;
        for (int t = tid; t < NN; t += NT) {
            const int i = t / N, j = t - i * N;
            const double v = uc[i] * K[i * P + j] * vc[j];
            if (!(fabs(v) < __builtin_inf())) bad = 1;
            Tk[i * P + j] = v;
        }
        __syncthreads();
    }
    if (c.chk)
        for (int t = tid; t < NN; t += NT) { const int i = t / N, j = t - i * N; c.chk[(size_t)b * NN + t] = (float)Tk[i * P + j]; }
    const bool flagged = __syncthreads_or(bad) != 0 || (fwd_flags & 4) != 0;                                            // (workgroup-uniform)
    if (c.binfo && tid == 0) {
        c.binfo[b * 2 + 0] = sk_total;
        c.binfo[b * 2 + 1] = (sk_total != c.info[b * 4 + 1] ? 1 : 0) | (flagged ? 4 : 0);
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
        const double dd = (double)c.ddist[b];
        line_sums(false, [&](int, int, int o) { return Tk[o]; }, zc);      // r = T 1
        line_sums(true, [&](int, int, int o) { return Tk[o]; }, wc);       // c = T^T 1
        for (int l = tid; l < N; l += NT) {
            double s1 = 0.0, s2 = 0.0;
            for (int i = 0; i < N; ++i) {
                const double a = (double)C1g[i * N + l], e = (double)C2g[i * N + l];
                s1 += a * a * zc[i]; s2 += e * e * wc[i];
            }
            dpa[l] = dd * alpha * s1; dqa[l] = dd * alpha * s2;
        }
        mm_f64_glb<NW, false>(N, N, N, C1g, N, Tk, P, [&](int i, int j, double v) { A[i * P + j] = v; });              // C1 T
        for (int t = tid; t < NN; t += NT) { const int i = t / N, j = t - i * N; dMa[t] = dd * om * Tk[i * P + j]; }
        __syncthreads();
        mm_f64_glb<NW, true>(N, N, N, A, P, C2g, N, [&](int i, int j, double g) {                                      // C1 T C2^T
            const double dx = dTg ? (double)dTg[i * N + j] : 0.0;
            Gb[i * P + j] = dx + dd * (om * (double)Mg[i * N + j] + alpha * (c0[i] + r0[j]) - two_alpha * g);
        });
        mm_f64_pad<NW>(N, N, N, [&](int j, int k) { return Tk[k * P + j]; }, [&](int k, int l) { return A[k * P + l]; }, [&](int j, int l, double v) {
            dC2a[j * N + l] = dd * two_alpha * ((double)C2g[j * N + l] * wc[j] * qb[l] - v);                            // T^T C1 T
        });
        __syncthreads();
        mm_f64_glb<NW, false>(N, N, N, Tk, P, C2g, N, [&](int i, int j, double v) { A[i * P + j] = v; });              // T C2
        __syncthreads();
        mm_f64_glb<NW, true>(N, N, N, A, P, Tk, P, [&](int i, int l, double v) {
            dC1a[i * N + l] = dd * two_alpha * ((double)C1g[i * N + l] * zc[i] * pa[l] - v);                            // T C2 T^T
        });
        mm_f64_pad<NW>(N, N, N, [&](int i, int k) { return (double)C1g[k * N + i]; }, [&](int k, int j) { return A[k * P + j]; }, [&](int i, int j, double v) {
            Gb[i * P + j] = live(i, j) ? Gb[i * P + j] - dd * two_alpha * v : 0.0;                                      // C1^T T C2
        });
    } else {
        for (int t = tid; t < NN; t += NT) {
            const int i = t / N, j = t - i * N;
            Gb[i * P + j] = live(i, j) ? (double)dTg[t] : 0.0;
            dMa[t] = 0.0; dC1a[t] = 0.0; dC2a[t] = 0.0;
        }
    }
    __syncthreads();

    // ---- step 2b: the outer iterations in reverse --------------------------------------------------------------------------------------------------
    for (int k = iters - 1; k >= 0; --k) {
        const double *xr = rec + (size_t)k * NN;
        for (int t = tid; t < NN; t += NT) { const int i = t / N, j = t - i * N; Tk[i * P + j] = xr[t]; }
        __syncthreads();
        form_K();                                                           // A = C1 Tk (symmetric) or C1^T Tk
        const int S = __builtin_amdgcn_readfirstlane(min(max(srec[k], 1), nim));
        sweeps(false, S, true);
        // the Sinkhorn reverse sweeps: plan cotangent Gb, loss cotangent 0
        line_sums(false, [&](int l, int e, int o) { return Gb[o] * (uc[l] * K[o] * vc[e]); }, fb);
        line_sums(true, [&](int l, int e, int o) { return Gb[o] * (uc[e] * K[o] * vc[l]); }, gb);
        for (int i = tid; i < N; i += NT) { la[i] = 0.0; lb[i] = 0.0; }
        for (int t = S; t >= 1; --t) {
            const double *ut = hU + (size_t)t * N, *up = ut - N, *vt = hV + (size_t)t * N;
            for (int i = tid; i < N; i += NT) {
                const double f = fb[i], z = pa[i] > 0.0 ? f * ut[i] / pa[i] : 0.0;
                la[i] += f; zc[i] = z; hZ[(size_t)(t - 1) * N + i] = z;
            }
            __syncthreads();
            line_sums(true, [&](int, int e, int o) { return K[o] * zc[e]; }, wc);
            for (int j = tid; j < N; j += NT) {
                const double g = gb[j] - vt[j] * wc[j], w = qb[j] > 0.0 ? g * vt[j] / qb[j] : 0.0;
                lb[j] += g; gb[j] = 0.0; wc[j] = w; hW[(size_t)(t - 1) * N + j] = w;
            }
            __syncthreads();
            line_sums(false, [&](int, int e, int o) { return K[o] * wc[e]; }, fb);
            for (int i = tid; i < N; i += NT) fb[i] = -up[i] * fb[i];
            __syncthreads();
        }
        // D = d tens = -(Gb o T_(k+1) - K o sum_t [z^t v^t^T + u^(t-1) w^t^T]) / eps
        mm_f64_pad<NW>(N, N, 2 * S,
                       [&](int i, int kk) { return kk < S ? hZ[(size_t)kk * N + i] : hU[(size_t)(kk - S) * N + i]; },
                       [&](int kk, int j) { return kk < S ? hV[(size_t)(kk + 1) * N + j] : hW[(size_t)(kk - S) * N + j]; },
                       [&](int i, int j, double v) {
                           const int o = i * P + j;
                           const double kij = K[o];
                           D[o] = -(Gb[o] * (uc[i] * kij * vc[j]) - kij * v) / eps;
                       });
        for (int i = tid; i < N; i += NT) {
            if (pa[i] > 0.0) dpa[i] += la[i] / pa[i];
            if (qb[i] > 0.0) dqa[i] += lb[i] / qb[i];
        }
        __syncthreads();
        line_sums(false, [&](int, int, int o) { return D[o]; }, zc);       // rho
        line_sums(true, [&](int, int, int o) { return D[o]; }, wc);        // kappa
        for (int t = tid; t < NN; t += NT) { const int i = t / N, j = t - i * N; dMa[t] += om * D[i * P + j]; }
        for (int l = tid; l < N; l += NT) {
            double s1 = 0.0, s2 = 0.0;
            for (int i = 0; i < N; ++i) {
                const double a = (double)C1g[i * N + l], e = (double)C2g[i * N + l];
                if (sym) { s1 += a * a * zc[i]; s2 += e * e * wc[i]; }
                else {
                    const double at = (double)C1g[l * N + i], et = (double)C2g[l * N + i];
                    s1 += (a * a + at * at) * zc[i]; s2 += (e * e + et * et) * wc[i];
                }
            }
            dpa[l] += (sym ? two_alpha : alpha) * s1; dqa[l] += (sym ? two_alpha : alpha) * s2;
        }
        auto next_gb = [&](int i, int j, double v) {                       // the cotangent of T_k, v: its product terms with their factor
            const int o = i * P + j;
            Gb[o] = live(i, j) ? v - (ppa ? eps * D[o] / Tk[o] : 0.0) : 0.0;
        };
        if (sym) {
            mm_f64_pad<NW>(N, N, N, [&](int j, int kk) { return D[kk * P + j]; }, [&](int kk, int l) { return A[kk * P + l]; }, [&](int j, int l, double v) {
                dC2a[j * N + l] += four_alpha * ((double)C2g[j * N + l] * wc[j] * qb[l] - v);                           // D^T (C1 Tk)
            });
            __syncthreads();
            mm_f64_glb<NW, false>(N, N, N, D, P, C2g, N, [&](int i, int j, double v) { A[i * P + j] = v; });           // D C2
            __syncthreads();
            mm_f64_glb<NW, true>(N, N, N, A, P, Tk, P, [&](int i, int l, double v) {
                dC1a[i * N + l] += four_alpha * ((double)C1g[i * N + l] * zc[i] * pa[l] - v);                           // D C2 Tk^T
            });
            mm_f64_pad<NW>(N, N, N, [&](int i, int kk) { return (double)C1g[kk * N + i]; }, [&](int kk, int j) { return A[kk * P + j]; },
                           [&](int i, int j, double v) { next_gb(i, j, -four_alpha * v); });                            // C1^T D C2
        } else {
            mm_f64_pad<NW>(N, N, N, [&](int j, int kk) { return A[kk * P + j]; }, [&](int kk, int l) { return D[kk * P + l]; }, [&](int j, int l, double v) {
                dC2a[j * N + l] += two_alpha * ((double)C2g[j * N + l] * (wc[j] * qb[l] + qb[j] * wc[l]) - v);          // Tk^T C1 D
            });
            __syncthreads();
            mm_f64_glb<NW, false>(N, N, N, C1g, N, Tk, P, [&](int i, int j, double v) { A[i * P + j] = v; });          // C1 Tk
            __syncthreads();
            mm_f64_pad<NW>(N, N, N, [&](int j, int kk) { return D[kk * P + j]; }, [&](int kk, int l) { return A[kk * P + l]; },
                           [&](int j, int l, double v) { dC2a[j * N + l] -= two_alpha * v; });                          // D^T C1 Tk
            __syncthreads();
            mm_f64_glb<NW, false>(N, N, N, D, P, C2g, N, [&](int i, int j, double v) { A[i * P + j] = v; });           // D C2
            __syncthreads();
            mm_f64_glb<NW, true>(N, N, N, A, P, Tk, P, [&](int i, int l, double v) {
                dC1a[i * N + l] += two_alpha * ((double)C1g[i * N + l] * (zc[i] * pa[l] + pa[i] * zc[l]) - v);          // D C2 Tk^T
            });
            mm_f64_pad<NW>(N, N, N, [&](int i, int kk) { return (double)C1g[kk * N + i]; }, [&](int kk, int j) { return A[kk * P + j]; },
                           [&](int i, int j, double v) { Gb[i * P + j] = -two_alpha * v; });                            // C1^T D C2
            __syncthreads();
            mm_f64_glb<NW, true>(N, N, N, D, P, C2g, N, [&](int i, int j, double v) { A[i * P + j] = v; });            // D C2^T
            __syncthreads();
            mm_f64_glb<NW, true>(N, N, N, Tk, P, A, P, [&](int i, int l, double v) { dC1a[i * N + l] -= two_alpha * v; });      // Tk C2 D^T
            mm_f64_glb<NW, false>(N, N, N, C1g, N, A, P, [&](int i, int j, double v) { next_gb(i, j, Gb[i * P + j] - two_alpha * v); });      // C1 D C2^T
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

int conan_fgw_pair_bwd_lds_resident(int N) { return N > 0 && PairStore::resident(N) ? 1 : 0; }

long long conan_fgw_pair_bwd_workspace_bytes(int B, int N, int max_iter, int num_iter_max) {
    if (B <= 0 || max_iter <= 0 || num_iter_max <= 0 || !PairStore::supported(N)) return 0;
    return (long long)((size_t)B * pgb_stride(N, max_iter, num_iter_max));
}

int conan_fgw_pair_bwd(const float *M, const float *C1, const float *C2, const float *p, const float *q, const float *G0, int B, int N, double alpha,
                       double epsilon, int max_iter, int num_iter_max, double stop_thr, int solver, int symmetric, const int *info, const float *dT,
                       const float *ddist, float *dM, float *dC1, float *dC2, float *dp, float *dq, float *dG0, float *T_chk, int *binfo,
                       void *workspace, void *stream) {
    PairBwdCall c{};
    static_cast<UnrollPairIO &>(c) = {M, C1, C2, p, q, G0, info, dT, ddist, dM, dC1, dC2, dp, dq, dG0, T_chk};
    if (max_iter <= 0 || num_iter_max <= 0 || unroll_pair_args(c, B, N, workspace, epsilon, alpha) != CONAN_OK || !(stop_thr == stop_thr)) return CONAN_E_BADARG;
    if (solver < 0 || solver > 1 || symmetric < -1 || symmetric > 1) return CONAN_E_BADARG;
    if (!PairStore::supported(N)) return CONAN_E_UNSUPPORTED;
    c.binfo = binfo;
    c.N = N; c.P = pitch_of(N); c.max_iter = max_iter; c.num_iter_max = num_iter_max; c.ppa = solver == 1; c.symmetric = symmetric;
    c.alpha = alpha; c.eps = epsilon; c.stop_thr = stop_thr;
    c.ws = static_cast<char *>(workspace); c.ws_stride = pgb_stride(N, max_iter, num_iter_max);
    if (PairStore::resident(N)) launch_lds(k_fgw_pair_bwd<true>, B, 64 * UNROLL_NW, PairStore::lds_bytes(N), as_stream(stream), c);
    else launch_lds(k_fgw_pair_bwd<false>, B, 64 * UNROLL_NW, PairStore::lds_bytes(N), as_stream(stream), c);
    CONAN_LAUNCH_CHECK();
    return CONAN_OK;
}

}  // extern "C"
