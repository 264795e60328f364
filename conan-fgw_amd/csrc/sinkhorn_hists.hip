// Sinkhorn-Knopp for several target histograms at once on gfx950: the reference's sinkhorn_knopp with b [n2, H] (sinkhorn.py:207-315), its
// one-to-many form: one cost matrix, one source histogram a, H target histograms, H transport costs, ONE stop for all of them
// (conan_sinkhorn_hists_fwd; DESIGN.md 3.3, "Several histograms at once"), and the fixed-plan gradient of those costs to M
// (conan_sinkhorn_hists_loss_bwd).  B problems per launch, one workgroup of SKH_NW wavefronts per problem.
//
// Sizes.  Problem p is n1[p] x n2[p] with nh[p] histograms (device-side, nullable: N1, N2, H) inside the containers [N1, N2], [N2, H].  Every loop
// runs over the problem's own rows, columns and histograms, K has the problem's own pitch P = n2[p] | 1, the scaling matrices the pitch
// HP = nh[p] | 1, and nothing outside the block is read.  Outputs outside the block are written as zeros.
//
// Arithmetic.  fp32 in and out, fp64 in between.  K = exp((double)M / -reg) is formed once, as k_sinkhorn's Knopp branch forms it.  The scaling
// vectors are matrices U [n1, HP], V [n2, HP], and a sweep is two products against K, each reading K once for all histograms:
//     column pass   S = K^T U,          V = b / S                         [n2 x n1] @ [n1 x nh]
//     row pass      R = ((1 / a) K) V,  U = 1 / R                         [n1 x n2] @ [n2 x nh]      (the reference's Kp @ v: same fp64 factors)
//     check (ii % 10 == 0)   err = || V o (K^T U) - b ||_F over all n2 nh entries, stop when err < stop_thr: one stop for every histogram
// Numerical-errors exit (sinkhorn.py:262-274): a zero entry of S, a NaN or Inf in U or V, in ANY histogram, restores the previous U, V of ALL
// histograms (they are double-buffered), raises flag bit 1 and leaves the loop.  A zero entry of a gives u_i = 1 / inf = 0, a zero entry of b
// v_jk = 0, as in k_sinkhorn's Knopp branch.
// The costs are loss_k = sum_i u_ik (sum_j (K o M)_ij v_jk): a third product of the same shape, then one column sum per histogram.
//
// Products.  nh > SKH_DOT_MAX: fgw_common.h's padded-tile product on v_mfma_f64_16x16x4_f64 (mm_f64_pad): a 16-wide tile of histograms costs
// what one costs, K is the A operand (lane <-> 16 consecutive columns resp. 16 rows at the odd pitch P: conflict-free), U / V the B operand.
// nh <= SKH_DOT_MAX: one wavefront per output row, lane <-> k, nh register accumulators fed from ONE read of K, then nh butterflies: a tile
// would be three quarters empty, and the tiles of a 33-row problem (3 x 1) leave one of the four wavefronts idle.  The path depends on nh[p]
// alone, and every sum has a fixed order (a tile's one accumulator chain in k order; per lane in index order, then the xor butterfly; for the
// error the storing lanes' own entries in tile order, the butterfly, the wavefronts in order): no atomics, nothing shared between workgroups,
// every loop bounded by num_iter_max.  A problem gives the same bits alone, in any batch, at any position and in any container, LDS-resident
// or streamed.
//
// Storage.  U, V, their previous values, b and 1 / a live in LDS: (16 + N1 + (2 N1 + 3 N2) (H | 1)) * 8 bytes, which bounds the supported
// (N1, N2, H) (conan_sinkhorn_hists_max_hists).  K lives in LDS when the CONTAINER fits next to them (conan_sinkhorn_hists_lds_resident), else
// every problem of the launch streams it from its slice of the workspace, as k_sinkhorn<false> does.
#include "fgw_common.h"
#include "../../include/conan_fgw_hip_sinkhorn_hists.h"
namespace {
constexpr int SKH_NW = 4, SKH_NT = 64 * SKH_NW;
constexpr int SKH_DOT_MAX = 4;      // histograms up to which a product runs as per-wavefront dots

struct SkhCall {
    const float *M, *a, *b, *wu, *wv;
    const int *n1, *n2, *nh;
    int N1, N2, H, num_iter_max, nerr;
    long long m_stride;
    double reg, stop_thr;
    float *loss, *log_u, *log_v, *errs;
    int *info;
    double *ws;
    size_t ws_stride;               // doubles per problem
};

struct SkhBwdCall {
    const float *M, *log_u, *log_v, *g;
    const int *n1, *n2, *nh;
    int N1, N2, H;
    long long m_stride;
    double reg;
    float *dM;
};

inline size_t skh_vec_bytes(int N1, int N2, int H) { return (16 + (size_t)N1 + (2 * (size_t)N1 + 3 * (size_t)N2) * (size_t)(H | 1)) * 8; }
inline size_t skh_mat_bytes(int N1, int N2) { return (size_t)N1 * (size_t)(N2 | 1) * 8; }
inline size_t skh_bwd_bytes(int N1, int N2, int H) { return ((size_t)N1 + (size_t)N2) * (size_t)(H | 1) * 8; }
inline bool skh_supported(int N1, int N2, int H) {
    return N1 > 0 && N2 > 0 && H > 0 && (size_t)(2 * (size_t)N1 + 3 * (size_t)N2) * (size_t)(H | 1) < (size_t)1 << 24 &&
           skh_vec_bytes(N1, N2, H) <= LDS_LIMIT && skh_mat_bytes(N1, N2) / 8 < (size_t)1 << 31;
}

__device__ __forceinline__ bool skh_naninf(double x) { return !(fabs(x) < __builtin_inf()); }

// D[R x nh] = X[R x Kd] @ W[Kd x nh]: X(r, k) an element reader, W row-major in LDS with pitch HP, st(r, h, value) the writer (called by the lane
// that holds the value).  Workgroup-collective, no barrier inside.
template <class FX, class FS>
__device__ __forceinline__ void skh_prod(int R, int nh, int Kd, FX X, const double *__restrict__ W, int HP, FS st) {
    if (nh > SKH_DOT_MAX) {                                                // (workgroup-uniform)
        mm_f64_pad<SKH_NW>(R, nh, Kd, X, [&](int k, int h) { return W[k * HP + h]; }, st);
        return;
    }
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    for (int r = wave; r < R; r += SKH_NW) {
        double acc[SKH_DOT_MAX];
#pragma unroll
        for (int h = 0; h < SKH_DOT_MAX; ++h) acc[h] = 0.0;
        for (int k = lane; k < Kd; k += 64) {
            const double x = X(r, k);
#pragma unroll
            for (int h = 0; h < SKH_DOT_MAX; ++h)
                if (h < nh) acc[h] += x * W[k * HP + h];
        }
#pragma unroll
        for (int h = 0; h < SKH_DOT_MAX; ++h)
            if (h < nh) {
                const double s = wave_sum_d(acc[h]);
                if (lane == 0) st(r, h, s);
            }
    }
}

template <bool RES>
__global__ void __launch_bounds__(SKH_NT) k_sinkhorn_hists(SkhCall c) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int N1 = c.N1, N2 = c.N2, H = c.H, HC = H | 1;
    const int m1 = __builtin_amdgcn_readfirstlane(min(max(c.n1 ? c.n1[p] : N1, 0), N1));
    const int m2 = __builtin_amdgcn_readfirstlane(min(max(c.n2 ? c.n2[p] : N2, 0), N2));
    const int nh = __builtin_amdgcn_readfirstlane(min(max(c.nh ? c.nh[p] : H, 0), H));
    const int P = m2 | 1, HP = nh | 1, mm = m1 * m2;
    double *red = reinterpret_cast<double *>(smem);
    int *flag = reinterpret_cast<int *>(red + 14);                        // one slot per iteration parity; never cleared: a set flag ends the loop
    double *iav = red + 16, *u0 = iav + N1, *u1 = u0 + (size_t)N1 * HC, *bv = u1 + (size_t)N1 * HC, *v0 = bv + (size_t)N2 * HC, *v1 = v0 + (size_t)N2 * HC;
    double *K;
    if constexpr (RES) K = v1 + (size_t)N2 * HC;
    else K = c.ws + (size_t)p * c.ws_stride;
    const float *M = c.M + (size_t)p * (size_t)c.m_stride;
    float *errs = c.errs ? c.errs + (size_t)p * c.nerr : nullptr;
    float *log_u = c.log_u + (size_t)p * N1 * H, *log_v = c.log_v + (size_t)p * N2 * H, *loss = c.loss + (size_t)p * H;
    const double reg = c.reg;

    // padding of the containers and the untouched checks
    for (int t = tid; t < N1 * H; t += SKH_NT) { const int i = t / H, h = t - i * H; if (i >= m1 || h >= nh) log_u[t] = 0.f; }
    for (int t = tid; t < N2 * H; t += SKH_NT) { const int j = t / H, h = t - j * H; if (j >= m2 || h >= nh) log_v[t] = 0.f; }
    if (errs) for (int t = tid; t < c.nerr; t += SKH_NT) errs[t] = __builtin_nanf("");
    if (m1 == 0 || m2 == 0 || nh == 0) {                                  // (workgroup-uniform)
        if (c.info && tid < 4) c.info[p * 4 + tid] = 0;
        for (int h = tid; h < H; h += SKH_NT) loss[h] = 0.f;
        return;
    }
    for (int h = nh + tid; h < H; h += SKH_NT) loss[h] = 0.f;

    for (int i = tid; i < m1; i += SKH_NT) iav[i] = 1.0 / (c.a ? (double)c.a[(size_t)p * N1 + i] : 1.0 / (double)m1);
    for (int t = tid; t < m2 * nh; t += SKH_NT) {
        const int j = t / nh, h = t - j * nh;
        const size_t g = (size_t)p * N2 * H + (size_t)j * H + h;
        bv[j * HP + h] = (double)c.b[g];
        v0[j * HP + h] = c.wv ? exp((double)c.wv[g]) : 1.0 / (double)m2;
    }
    for (int t = tid; t < m1 * nh; t += SKH_NT) {
        const int i = t / nh, h = t - i * nh;
        u0[i * HP + h] = c.wu ? exp((double)c.wu[(size_t)p * N1 * H + (size_t)i * H + h]) : 1.0 / (double)m1;
    }
    for (int t = tid; t < mm; t += SKH_NT) {
        const int i = t / m2, j = t - i * m2;
        K[i * P + j] = exp((double)M[(size_t)i * N2 + j] / -reg);
    }
    if (tid < 2) flag[tid] = 0;
    __syncthreads();

    const auto Kt = [&](int j, int i) { return K[i * P + j]; };           // K^T as the left operand of the column pass
    const auto Kp = [&](int i, int j) { return iav[i] * K[i * P + j]; };  // the reference's Kp = (1 / a) K
    int ii = 0, flags = 0, nchk = 0, cur = 0;
    for (; ii < c.num_iter_max; ++ii) {
        const double *uo = cur ? u1 : u0;
        double *un = cur ? u0 : u1, *vn = cur ? v0 : v1;
        int *fl = flag + (ii & 1);
        skh_prod(m2, nh, m1, Kt, uo, HP, [&](int j, int h, double s) {   // v = b / (K^T u)                                 (sinkhorn.py:258-259)
            const double v = bv[j * HP + h] / s;
            vn[j * HP + h] = v;
            if (s == 0.0 || skh_naninf(v)) *fl = 1;
        });
        __syncthreads();
        skh_prod(m1, nh, m2, Kp, vn, HP, [&](int i, int h, double s) {   // u = 1 / (Kp v)                                   (sinkhorn.py:260)
            const double u = 1.0 / s;
            un[i * HP + h] = u;
            if (skh_naninf(u)) *fl = 1;
        });
        __syncthreads();
        if (*fl != 0) { flags |= 2; break; }                              // (workgroup-uniform) numerical errors: the previous u, v stay current
        cur ^= 1;
        if (ii % 10 == 0) {                                               // the joint violation of the column marginals     (sinkhorn.py:275-288)
            double e2 = 0.0;
            skh_prod(m2, nh, m1, Kt, un, HP, [&](int j, int h, double s) {
                const double d = vn[j * HP + h] * s - bv[j * HP + h];
                e2 += d * d;
            });
            const double err = sqrt(block_sum_d<SKH_NW>(e2, red));        // (its barriers also order these reads before the next updates)
            if (errs && tid == 0) errs[ii / 10] = (float)err;
            ++nchk;
            if (err < c.stop_thr) { flags |= 1; break; }
        }
    }
    const double *u = cur ? u1 : u0, *v = cur ? v1 : v0;
    double *G = cur ? u0 : u1;                                            // the buffer that is not current: G = u o ((K o M) v)
    for (int t = tid; t < m1 * nh; t += SKH_NT) {
        const int i = t / nh, h = t - i * nh;
        log_u[(size_t)i * H + h] = (float)log(u[i * HP + h]);
    }
    for (int t = tid; t < m2 * nh; t += SKH_NT) {
        const int j = t / nh, h = t - j * nh;
        log_v[(size_t)j * H + h] = (float)log(v[j * HP + h]);
    }
    skh_prod(m1, nh, m2, [&](int i, int j) { return K[i * P + j] * (double)M[(size_t)i * N2 + j]; }, v, HP,
             [&](int i, int h, double s) { G[i * HP + h] = u[i * HP + h] * s; });
    __syncthreads();
    for (int h = wave; h < nh; h += SKH_NW) {                             // loss_k = sum_i G_ik
        double s = 0.0;
        for (int i = lane; i < m1; i += 64) s += G[i * HP + h];
        s = wave_sum_d(s);
        if (lane == 0) loss[h] = (float)s;
    }
    if (tid == 0 && c.info) {
        int *info = c.info + p * 4;
        info[0] = ii < c.num_iter_max ? ii : c.num_iter_max - 1;         // the reference's log["niter"]: the loop index at exit
        info[1] = flags; info[2] = nchk; info[3] = 0;
    }
}

// dM_ij = K_ij sum_k g_k u_ik v_jk from M, log u, log v: K is recomputed, g_k u_ik and v_jk are staged in LDS, no [H, N1, N2] tensor exists.
__global__ void __launch_bounds__(SKH_NT) k_sinkhorn_hists_bwd(SkhBwdCall c) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int p = blockIdx.x, tid = threadIdx.x;
    const int N1 = c.N1, N2 = c.N2, H = c.H;
    const int m1 = __builtin_amdgcn_readfirstlane(min(max(c.n1 ? c.n1[p] : N1, 0), N1));
    const int m2 = __builtin_amdgcn_readfirstlane(min(max(c.n2 ? c.n2[p] : N2, 0), N2));
    const int nh = __builtin_amdgcn_readfirstlane(min(max(c.nh ? c.nh[p] : H, 0), H));
    const int HP = nh | 1;
    double *gu = reinterpret_cast<double *>(smem), *ev = gu + (size_t)N1 * (H | 1);
    const float *M = c.M + (size_t)p * (size_t)c.m_stride;
    float *dM = c.dM + (size_t)p * N1 * N2;
    for (int t = tid; t < m1 * nh; t += SKH_NT) {
        const int i = t / nh, h = t - i * nh;
        gu[i * HP + h] = (double)c.g[(size_t)p * H + h] * exp((double)c.log_u[(size_t)p * N1 * H + (size_t)i * H + h]);
    }
    for (int t = tid; t < m2 * nh; t += SKH_NT) {
        const int j = t / nh, h = t - j * nh;
        ev[j * HP + h] = exp((double)c.log_v[(size_t)p * N2 * H + (size_t)j * H + h]);
    }
    __syncthreads();
    for (int t = tid; t < N1 * N2; t += SKH_NT) {
        const int i = t / N2, j = t - i * N2;
        float out = 0.f;
        if (i < m1 && j < m2) {
            double s = 0.0;
            for (int h = 0; h < nh; ++h) s += gu[i * HP + h] * ev[j * HP + h];
            out = (float)(exp((double)M[t] / -c.reg) * s);
        }
        dM[t] = out;
    }
}

}  // namespace

extern "C" {

int conan_sinkhorn_hists_max_hists(int N1, int N2) {
    if (N1 <= 0 || N2 <= 0) return 0;
    const size_t words = LDS_LIMIT / 8, fixed = 16 + (size_t)N1, per = 2 * (size_t)N1 + 3 * (size_t)N2;
    if (fixed + per > words) return 0;
    const size_t hc = (words - fixed) / per;                               // the largest H | 1 that fits
    const int h = (int)(hc > 65535 ? 65535 : hc);
    return (h & 1) ? h : h - 1;                                            // (H | 1) <= hc: an odd hc admits H = hc, an even one H = hc - 1
}

int conan_sinkhorn_hists_lds_resident(int N1, int N2, int H) {
    if (!skh_supported(N1, N2, H)) return 0;
    return skh_vec_bytes(N1, N2, H) + skh_mat_bytes(N1, N2) <= LDS_LIMIT ? 1 : 0;
}

long long conan_sinkhorn_hists_workspace_bytes(int B, int N1, int N2, int H) {
    if (B <= 0 || !skh_supported(N1, N2, H)) return 0;
    if (conan_sinkhorn_hists_lds_resident(N1, N2, H)) return 256;          // nothing is streamed; a non-empty buffer keeps the pointer valid
    return (long long)((size_t)B * al256(skh_mat_bytes(N1, N2)));
}

int conan_sinkhorn_hists_fwd(const float *M, const float *a, const float *b, const float *warm_u, const float *warm_v, const int *n1, const int *n2,
                             const int *nh, int B, int N1, int N2, int H, long long m_batch_stride, double reg, int num_iter_max, double stop_thr,
                             float *loss, float *log_u, float *log_v, int *info, float *errs, void *workspace, void *stream) {
    if (!M || !b || !loss || !log_u || !log_v || !workspace || B <= 0 || N1 <= 0 || N2 <= 0 || H <= 0 || num_iter_max <= 0 || m_batch_stride < 0)
        return CONAN_E_BADARG;
    if ((warm_u == nullptr) != (warm_v == nullptr)) return CONAN_E_BADARG;
    if (!(reg > 0.0) || !(reg < __builtin_inf()) || !(stop_thr == stop_thr)) return CONAN_E_BADARG;
    if (!skh_supported(N1, N2, H)) return CONAN_E_UNSUPPORTED;
    SkhCall c{};
    c.M = M; c.a = a; c.b = b; c.wu = warm_u; c.wv = warm_v; c.n1 = n1; c.n2 = n2; c.nh = nh;
    c.N1 = N1; c.N2 = N2; c.H = H; c.num_iter_max = num_iter_max; c.nerr = (num_iter_max + 9) / 10;
    c.m_stride = m_batch_stride; c.reg = reg; c.stop_thr = stop_thr;
    c.loss = loss; c.log_u = log_u; c.log_v = log_v; c.errs = errs; c.info = info;
    c.ws = static_cast<double *>(workspace); c.ws_stride = al256(skh_mat_bytes(N1, N2)) / 8;
    const hipStream_t s = as_stream(stream);
    const size_t vec = skh_vec_bytes(N1, N2, H);
    if (conan_sinkhorn_hists_lds_resident(N1, N2, H)) launch_lds(k_sinkhorn_hists<true>, B, SKH_NT, vec + skh_mat_bytes(N1, N2), s, c);
    else launch_lds(k_sinkhorn_hists<false>, B, SKH_NT, vec, s, c);
    CONAN_LAUNCH_CHECK();
    return CONAN_OK;
}

int conan_sinkhorn_hists_loss_bwd(const float *M, const float *log_u, const float *log_v, const float *g, const int *n1, const int *n2, const int *nh,
                                  int B, int N1, int N2, int H, long long m_batch_stride, double reg, float *dM, void *stream) {
    if (!M || !log_u || !log_v || !g || !dM || B <= 0 || N1 <= 0 || N2 <= 0 || H <= 0 || m_batch_stride < 0) return CONAN_E_BADARG;
    if (!(reg > 0.0) || !(reg < __builtin_inf())) return CONAN_E_BADARG;
    if (!skh_supported(N1, N2, H)) return CONAN_E_UNSUPPORTED;
    SkhBwdCall c{};
    c.M = M; c.log_u = log_u; c.log_v = log_v; c.g = g; c.n1 = n1; c.n2 = n2; c.nh = nh;
    c.N1 = N1; c.N2 = N2; c.H = H; c.m_stride = m_batch_stride; c.reg = reg; c.dM = dM;
    launch_lds(k_sinkhorn_hists_bwd, B, SKH_NT, skh_bwd_bytes(N1, N2, H), as_stream(stream), c);
    CONAN_LAUNCH_CHECK();
    return CONAN_OK;
}

}  // extern "C"
