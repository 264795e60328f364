// FGWMixup's coupling solve for gfx950: the reference's fused_ACC_torch (barycenter.py:228-256), an accelerated mirror descent, on its own
// (the pair form, conan_fgw_acc_pair_fwd) and as the coupling solve of fgw_barycenters_BAPG (barycenter.py:259-390, the barycenter form,
// conan_fgw_mixup_barycenter_fwd).  This is NOT solver="BAPG" of fgw_barycenters (fgw_bapg.hip, the reference's fgw_bregman): the gradient
// differs, the iterate is lifted by 1e-10 every epoch and the stop is on the relative change of an objective.
//
// One workgroup per coupling (grid B*K, or B pairs).  One epoch, ii = 0 .. epoch - 1, with X0 = a b^T:
//
//     X <- X + 1e-10
//     X <- X * exp((4 alpha (A X) B - (1 - alpha) M) / rho);  X <- diag(a / rowsum X) X
//     X <- X * exp((4 alpha (A X) B - (1 - alpha) M) / rho);  X <- X diag(b / colsum X)
//     ii > 0 and ii % 10 == 0:  obj = sum(((1 - alpha) M - 2 alpha (A X) B) * X); stop when |obj - last| / |last| < eps, else keep obj as last
//
// so the first check (ii = 10) only stores, the earliest stop is after 21 epochs, and a NaN objective never stops the loop.  B enters
// UNTRANSPOSED (the Bregman solve multiplies by C2^T): directed graphs give another product.  The two N^3 products per half-step run on fp64
// MFMA (mm_f64_glb); every sum has a fixed order, there are no atomics except the two info words of the barycenter form, and every loop is
// bounded by `epoch`.
//
// Matrices (pitch P, fp64): X, AX = A X and Mb = (1 - alpha) M, 24 bytes per entry: in LDS while they fit (conan_fgw_acc_lds_resident), else in
// the coupling's slice of the global scratch (28 bytes per entry, as the other coupling kernels lay it out).  A and B are read from global
// memory by the products.
//
// Nodes without mass (other sizes are embedded in a square problem with such nodes): an entry whose row or column has no mass stays exactly
// zero — the 1e-10 is not added there and its scaling factor is 0 — so the embedded problem is the reference's rectangular one.  A row or
// column WITH mass whose sum is zero (exp underflow) or not finite (overflow) gives the reference's NaN; flags bit 2 is raised and the solve
// still runs to its end.
//
// The epochs themselves (acc_epochs, with the sizes and the LDS carve) are in fgw_acc_body.h: the unrolled gradient (fgw_acc_grad.hip) replays
// them from the same text.
#include "fgw_acc_body.h"
#include "../../include/conan_fgw_hip_mixup_grad.h"

namespace {

// ------------------------------------------------------------------------------------------------ the barycenter form
// Takes the place of the coupling kernel in the outer loop of the barycenter solve and hands the update stage (k_fgw_update_parts) the same
// things: T, Ypart = T Z, Cpart = T h(C2) T^T with h = identity (square loss) or log(max(., 1e-15)) (kl).  Always starts from p ps[s]^T.
template <bool LDS, bool KL>
__global__ void __launch_bounds__(64 * ACC_NW) k_fgw_acc_coupling(
    const float *__restrict__ Ys, const float *__restrict__ Cs, const float *__restrict__ ps, const float *__restrict__ pb, FgwDims D,
    conan_fgw_params prm, double rho, int epoch, double eps, int outer, int y_zero, const double *__restrict__ Cw, const double *__restrict__ Yw,
    const int *__restrict__ active, float *__restrict__ Tw, int *__restrict__ info, char *__restrict__ scratch, size_t scratch_stride,
    fgw_part_t *__restrict__ Ypart, fgw_part_t *__restrict__ Cpart) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int NW = ACC_NW, NT = 64 * NW;
    const int cid = blockIdx.x;
    const int b = cid / D.K, s = cid % D.K;
    if (!fgw_active(active, D.B, b, outer)) return;
    const int N = D.N, P = D.P, d = D.d, NN = N * N;
    const int tid = threadIdx.x;
    const AccCarve c = acc_carve<LDS>(smem, N, P, scratch + (size_t)cid * scratch_stride);
    double *pa = c.pa, *qb = c.qb, *y2a = c.y2a, *z2a = c.z2a, *X = c.X, *AX = c.AX, *Mb = c.Mb;

    const float *Z = Ys + ((size_t)b * D.K + s) * N * d;
    const float *C2 = Cs + ((size_t)b * D.K + s) * NN;
    const double *C1 = Cw + (size_t)b * NN;
    const double *Y = Yw + (size_t)b * N * d;
    float *Tg = Tw + ((size_t)b * D.K + s) * NN;
    const double alpha = (double)prm.alpha;

    // ---- marginals (uniform when not given) and squared feature norms
    for (int i = tid; i < N; i += NT) {
        pa[i] = pb ? (double)pb[(size_t)b * N + i] : 1.0 / (double)N;
        qb[i] = ps ? (double)ps[((size_t)b * D.K + s) * N + i] : 1.0 / (double)N;
    }
    {   // 8 lanes per index, strided partial sums combined by xor-shuffles (fixed order)
        constexpr int LPI = 8;
        for (int i0 = 0; i0 < N; i0 += NT / LPI) {
            const int i = i0 + tid / LPI, sub = tid % LPI;
            double y2 = 0.0, z2 = 0.0;
            if (i < N)
                for (int k = sub; k < d; k += LPI) {
                    const double yy = Y[i * d + k], zz = (double)Z[i * d + k];
                    y2 += yy * yy; z2 += zz * zz;
                }
#pragma unroll
            for (int o = 1; o < LPI; o <<= 1) { y2 += __shfl_xor(y2, o, 64); z2 += __shfl_xor(z2, o, 64); }
            if (i < N && sub == 0) { y2a[i] = y2; z2a[i] = z2; }
        }
    }
    __syncthreads();
    // ---- X0 = p ps[s]^T (no warm start, barycenter.py:344);  Mb = (1 - alpha) clamp(|y_i|^2 + |z_j|^2 - 2 y_i.z_j, 0)    (utils.py:154-171)
    for (int t = tid; t < NN; t += NT) { const int i = t / N, j = t - i * N; X[i * P + j] = pa[i] * qb[j]; }
    if (!y_zero) mm_f64_glb<NW, true>(N, N, d, Y, d, Z, d, [&](int i, int j, double v) { Mb[i * P + j] = v; });
    __syncthreads();
    for (int t = tid; t < NN; t += NT) {
        const int i = t / N, j = t - i * N;
        double m = -2.0 * (y_zero ? 0.0 : Mb[i * P + j]);
        m += y2a[i]; m += z2a[j];
        m = m > 0.0 ? m : 0.0;
        Mb[i * P + j] = (1.0 - alpha) * m;
    }
    __syncthreads();

    const AccProblem<double> q{C1, C2, alpha, rho, eps, epoch, nullptr};
    const AccResult r = acc_epochs(q, N, P, pa, qb, c.sc, c.pm, c.red, X, AX, Mb);

    if (r.zero_sum && tid == 0) atomicOr(&info[b * 4 + 3], 4);
    for (int t = tid; t < NN; t += NT) { const int i = t / N, j = t - i * N; Tg[t] = (float)X[i * P + j]; }
    if (tid == 0) atomicAdd(&info[b * 4 + 1], r.epochs);
    // ---- contributions to the barycenter update (summed over s by k_fgw_update_parts)
    if (!prm.fixed_features) {                                          // Ypart = T @ Z                      (utils.py:90-95)
        fgw_part_t *Yp = Ypart + ((size_t)b * D.K + s) * N * d;
        mm_f64_glb<NW, false>(N, d, N, X, P, Z, d, [&](int i, int k, double v) { Yp[(size_t)i * d + k] = (fgw_part_t)v; });
    }
    if (!prm.fixed_structure) {                                         // Cpart = T @ h(C2) @ T^T            (utils.py:67-87)
        fgw_part_t *Cp = Cpart + ((size_t)b * D.K + s) * NN;
        if constexpr (KL)
            mm_f64<NW>(N, N, N, [&](int i, int k) { return X[i * P + k]; },
                       [&](int k, int j) { const double cv = (double)C2[k * N + j]; return log(cv > 1e-15 ? cv : 1e-15); },
                       [&](int i, int j, double v) { AX[i * P + j] = v; });
        else
            mm_f64_glb<NW, false>(N, N, N, X, P, C2, N, [&](int i, int j, double v) { AX[i * P + j] = v; });
        __syncthreads();
        mm_f64_glb<NW, true>(N, N, N, AX, P, X, P, [&](int i, int j, double v) { Cp[i * N + j] = (fgw_part_t)v; });
    }
}

// ------------------------------------------------------------------------------------------------ the pair form
// M, A, Bm are the caller's, X0 (nullable) the start; info[b] = {epochs run, checks stored, flags, 0}.
template <bool LDS>
__global__ void __launch_bounds__(64 * ACC_NW) k_fgw_acc_pair(
    const float *__restrict__ M, const float *__restrict__ A, const float *__restrict__ Bm, const float *__restrict__ a, const float *__restrict__ bq,
    const float *__restrict__ X0, int N, int P, double alpha, double rho, int epoch, double eps, int nobj, float *__restrict__ Xout,
    float *__restrict__ objs, int *__restrict__ info, char *__restrict__ scratch, size_t scratch_stride) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int NT = 64 * ACC_NW;
    const int b = blockIdx.x, NN = N * N, tid = threadIdx.x;
    const AccCarve c = acc_carve<LDS>(smem, N, P, scratch + (size_t)b * scratch_stride);
    double *pa = c.pa, *qb = c.qb, *X = c.X, *Mb = c.Mb;
    const float *Mg = M + (size_t)b * NN, *Xs = X0 ? X0 + (size_t)b * NN : nullptr;
    for (int i = tid; i < N; i += NT) {
        pa[i] = a ? (double)a[(size_t)b * N + i] : 1.0 / (double)N;
        qb[i] = bq ? (double)bq[(size_t)b * N + i] : 1.0 / (double)N;
    }
    for (int k = tid; k < nobj; k += NT) objs[(size_t)b * nobj + k] = __builtin_nanf("");
    __syncthreads();
    for (int t = tid; t < NN; t += NT) {
        const int i = t / N, j = t - i * N;
        const double x0 = Xs ? (double)Xs[t] : pa[i] * qb[j];
        X[i * P + j] = (pa[i] > 0.0 && qb[j] > 0.0) ? x0 : 0.0;
        Mb[i * P + j] = (1.0 - alpha) * (double)Mg[t];
    }
    __syncthreads();
    const AccProblem<float> q{A + (size_t)b * NN, Bm + (size_t)b * NN, alpha, rho, eps, epoch, objs + (size_t)b * nobj};
    const AccResult r = acc_epochs(q, N, P, pa, qb, c.sc, c.pm, c.red, X, c.AX, Mb);
    for (int t = tid; t < NN; t += NT) { const int i = t / N, j = t - i * N; Xout[(size_t)b * NN + t] = (float)X[i * P + j]; }
    if (tid == 0) { info[b * 4 + 0] = r.epochs; info[b * 4 + 1] = r.stored; info[b * 4 + 2] = r.zero_sum ? 4 : 0; info[b * 4 + 3] = 0; }
}

// ------------------------------------------------------------------------------------------------ host side
// C <- init_C (or Cs[b,0]), Y <- init_Y (or 0), counters and flags: what k_fgw_init does for dense structure (that kernel is private to fgw.hip,
// whose object — the models' kernels — this feature leaves as it is)
__global__ void k_fgw_acc_init(const float *__restrict__ Cs, const float *__restrict__ init_C, const float *__restrict__ init_Y, FgwDims D,
                               int max_iter, double *__restrict__ Cw, double *__restrict__ Yw, int *__restrict__ active, int *__restrict__ info,
                               float *__restrict__ errs, float *__restrict__ Yout, float *__restrict__ Cout) {
    const int b = blockIdx.x;
    const int NN = D.N * D.N, Nd = D.N * D.d;
    const float *c0 = init_C ? init_C + (size_t)b * NN : Cs + (size_t)b * D.K * NN;
    for (int t = threadIdx.x; t < NN; t += blockDim.x) { Cw[(size_t)b * NN + t] = (double)c0[t]; Cout[(size_t)b * NN + t] = c0[t]; }
    for (int t = threadIdx.x; t < Nd; t += blockDim.x) {
        const float y = init_Y ? init_Y[(size_t)b * Nd + t] : 0.f;                      // barycenter.py:317-318
        Yw[(size_t)b * Nd + t] = (double)y; Yout[(size_t)b * Nd + t] = y;
    }
    if (threadIdx.x == 0) { fgw_active_init(active, D.B, b); info[b * 4 + 0] = 0; info[b * 4 + 1] = 0; info[b * 4 + 2] = 0; info[b * 4 + 3] = 0; }
    for (int t = threadIdx.x; t < 2 * max_iter; t += blockDim.x) errs[(size_t)b * 2 * max_iter + t] = __builtin_nanf("");
}

// Byte offsets of the regions of conan_fgw_mixup_barycenter_fwd's workspace, in this order, and the total the size query returns.
struct AccWorkspace {
    size_t Cw, Yw, active, scratch, Ypart, Cpart, total;
};
AccWorkspace acc_workspace(int B, int K, int N, int d) {
    AccWorkspace w{};
    if (B <= 0 || K <= 0 || N <= 0 || d <= 0) return w;
    const size_t NN = (size_t)N * N, NP = (size_t)N * pitch_of(N), BK = (size_t)B * K;
    size_t end = 0;
    auto region = [&](size_t bytes) { const size_t at = end; end += bytes; return at; };
    w.Cw = region(al256((size_t)B * NN * 8));
    w.Yw = region(al256((size_t)B * N * d * 8));
    w.active = region(al256((size_t)B * 16));                       // [parity][features | structure][B] ints (fgw_active)
    w.scratch = region(al256(BK * coupling_scratch_stride(NP)));    // the couplings' matrices outside LDS
    w.Ypart = region(al256(BK * N * d * sizeof(fgw_part_t)));
    w.Cpart = region(al256(BK * NN * sizeof(fgw_part_t)));
    w.total = end;
    return w;
}

inline bool acc_bad_step(double rho, int epoch, double eps) { return !(rho > 0.0 && rho <= 1.79769313486231570815e308) || epoch <= 0 || !(eps == eps); }

}  // namespace

extern "C" {

int conan_fgw_acc_lds_resident(int N) { return N > 0 && acc_lds(N) <= ACC_LDS_LIMIT ? 1 : 0; }

long long conan_fgw_acc_pair_workspace_bytes(int B, int N) {
    if (B <= 0 || N <= 0) return 0;
    return (long long)al256((size_t)B * coupling_scratch_stride((size_t)N * pitch_of(N)));
}

int conan_fgw_acc_pair_fwd(const float *M, const float *A, const float *Bm, const float *a, const float *b, const float *X0, int B, int N,
                           double alpha, double rho, int epoch, double eps, float *X, float *objs, int *info, void *workspace, void *stream) {
    if (!M || !A || !Bm || !X || !objs || !info || !workspace || B <= 0 || N <= 0) return CONAN_E_BADARG;
    if (acc_bad_step(rho, epoch, eps) || !(alpha == alpha)) return CONAN_E_BADARG;
    const int P = pitch_of(N), nobj = (epoch + 9) / 10;
    const bool lds = acc_lds(N) <= ACC_LDS_LIMIT;
    const size_t stride = coupling_scratch_stride((size_t)N * P);
    with_flags([&](auto L) {
        launch_lds(k_fgw_acc_pair<L.value>, B, 64 * ACC_NW, lds ? acc_lds(N) : acc_vec_bytes(N), as_stream(stream), M, A, Bm, a, b, X0, N, P, alpha, rho,
                   epoch, eps, nobj, X, objs, info, static_cast<char *>(workspace), stride);
    }, lds);
    CONAN_LAUNCH_CHECK();
    return CONAN_OK;
}

long long conan_fgw_mixup_workspace_bytes(int B, int K, int N, int d) { return (long long)acc_workspace(B, K, N, d).total; }

}  // extern "C"

namespace {
// The outer loop of fgw_barycenters_BAPG: as fgw_fwd_impl queues it — init, then max_iter times coupling solve, snapshot, update — with no
// host synchronisation; a molecule that has converged leaves its workgroups at once (fgw_active).  record (nullable): the fp64 state after
// init and after every update, [max_iter + 1][B][N,N] then [max_iter + 1][B][N,d], copied device to device as T_iter is (the unrolled
// gradient, fgw_mixup_grad.hip, walks it back; a molecule that has converged keeps its state, so the later entries repeat its last one).
int acc_mixup_fwd(const float *Ys, const float *Cs, const float *ps, const float *p, const float *lambdas, const float *init_C,
                  const float *init_Y, int B, int K, int N, int d, const conan_fgw_params *params, double rho, int epoch, double eps,
                  float *Y, float *C, float *T, float *T_iter, int *info, float *errs, double *record, void *workspace, void *stream) {
    if (!Ys || !Cs || !params || !Y || !C || !T || !info || !errs || !workspace || B <= 0 || K <= 0 || N <= 0 || d <= 0) return CONAN_E_BADARG;
    if (params->max_iter <= 0 || acc_bad_step(rho, epoch, eps)) return CONAN_E_BADARG;
    if (params->fixed_features && !init_Y) return CONAN_E_BADARG;      // barycenter.py:311-313
    if (params->loss_fun != 0 && params->loss_fun != 1) return CONAN_E_BADARG;
    const AccWorkspace w = acc_workspace(B, K, N, d);
    const size_t NN = (size_t)N * N, NP = (size_t)N * pitch_of(N);
    FgwCall c{};
    c.Ys = Ys; c.Cs = Cs; c.ps = ps; c.p = p; c.lambdas = lambdas; c.init_C = init_C; c.init_Y = init_Y;
    c.D = FgwDims{B, K, N, d, pitch_of(N)};
    c.prm = *params;
    c.symmetric = 1;
    c.Y = Y; c.C = C; c.T = T; c.info = info; c.errs = errs;
    c.Cw = ws_at<double>(workspace, w.Cw); c.Yw = ws_at<double>(workspace, w.Yw); c.active = ws_at<int>(workspace, w.active);
    c.scratch = ws_at<char>(workspace, w.scratch); c.scratch_stride = coupling_scratch_stride(NP);
    c.Ypart = ws_at<fgw_part_t>(workspace, w.Ypart); c.Cpart = ws_at<fgw_part_t>(workspace, w.Cpart);
    c.s = as_stream(stream);
    const bool lds = acc_lds(N) <= ACC_LDS_LIMIT;
    const size_t bytes = lds ? acc_lds(N) : acc_vec_bytes(N);

    const size_t Nd = (size_t)N * d;
    double *Crec = record, *Yrec = record ? record + (size_t)(c.prm.max_iter + 1) * B * NN : nullptr;
    auto snapshot = [&](int t) {
        (void)hipMemcpyAsync(Crec + (size_t)t * B * NN, c.Cw, (size_t)B * NN * sizeof(double), hipMemcpyDeviceToDevice, c.s);
        (void)hipMemcpyAsync(Yrec + (size_t)t * B * Nd, c.Yw, (size_t)B * Nd * sizeof(double), hipMemcpyDeviceToDevice, c.s);
    };

    k_fgw_acc_init<<<B, 256, 0, c.s>>>(Cs, init_C, init_Y, c.D, c.prm.max_iter, c.Cw, c.Yw, c.active, info, errs, Y, C);
    if (record) snapshot(0);
    for (int outer = 0; outer < c.prm.max_iter; ++outer) {
        const int y_zero = (outer == 0 && !init_Y) ? 1 : 0;
        with_flags([&](auto L, auto KL) {
            launch_lds(k_fgw_acc_coupling<L.value, KL.value>, B * K, 64 * ACC_NW, bytes, c.s, Ys, Cs, ps, p, c.D, c.prm, rho, epoch, eps, outer, y_zero,
                       c.Cw, c.Yw, c.active, T, info, c.scratch, c.scratch_stride, c.Ypart, c.Cpart);
        }, lds, c.prm.loss_fun != 0);
        if (T_iter)      // log["Ts_iter"] (barycenter.py:373): a snapshot per outer iteration, only when the caller asks for the log
            (void)hipMemcpyAsync(T_iter + (size_t)outer * B * K * NN, T, (size_t)B * K * NN * sizeof(float), hipMemcpyDeviceToDevice, c.s);
        conan_fgw_small_update(c, outer, false);
        if (record) snapshot(outer + 1);
    }
    CONAN_LAUNCH_CHECK();
    return CONAN_OK;
}
}  // namespace

extern "C" {

int conan_fgw_mixup_barycenter_fwd(const float *Ys, const float *Cs, const float *ps, const float *p, const float *lambdas, const float *init_C,
                                   const float *init_Y, int B, int K, int N, int d, const conan_fgw_params *params, double rho, int epoch, double eps,
                                   float *Y, float *C, float *T, float *T_iter, int *info, float *errs, void *workspace, void *stream) {
    return acc_mixup_fwd(Ys, Cs, ps, p, lambdas, init_C, init_Y, B, K, N, d, params, rho, epoch, eps, Y, C, T, T_iter, info, errs, nullptr, workspace, stream);
}

// (declared in include/conan_fgw_hip_mixup_grad.h)
int conan_fgw_mixup_barycenter_fwd_record(const float *Ys, const float *Cs, const float *ps, const float *p, const float *lambdas, const float *init_C,
                                          const float *init_Y, int B, int K, int N, int d, const conan_fgw_params *params, double rho, int epoch,
                                          double eps, float *Y, float *C, float *T, float *T_iter, int *info, float *errs, void *record,
                                          void *workspace, void *stream) {
    if (!record) return CONAN_E_BADARG;
    return acc_mixup_fwd(Ys, Cs, ps, p, lambdas, init_C, init_Y, B, K, N, d, params, rho, epoch, eps, Y, C, T, T_iter, info, errs,
                         static_cast<double *>(record), workspace, stream);
}

}  // extern "C"
