// Full backward of the FGW barycenter block for gfx950: gradients for Ys, Cs, p, lambdas, init_C and init_Y given the saved couplings T.
//
// The reference solves the couplings under torch.no_grad() (barycenter.py:120); its last update steps are differentiable:
//
//     Y = diag(1/p) sum_s lam_s T_s Z_s                                        (update_feature_matrix, utils.py:90-95)
//     C = (sum_s lam_s T_s C2_s T_s^T) / (p p^T)                               (update_square_loss, utils.py:67-73)
//     C = exp((sum_s lam_s T_s log(max(C2_s, 1e-15)) T_s^T) / (p p^T))       (update_kl_loss, utils.py:76-87)
//     Y = init_Y / C = init_C under fixed_features / fixed_structure           (barycenter.py:56-80)
//
// With U = dL/dY, V = dL/dC, H = V / (p p^T) (square) or (V o C) / (p p^T) (KL), G_s = T_s^T H T_s:
//
//     dZ_s = lam_s T_s^T diag(1/p) U               dlam_s = <T_s^T diag(1/p) U, Z_s> + <G_s, C2_s or log max(C2_s, 1e-15)>
//     dC2_s = lam_s G_s  (KL: lam_s G_s / C2_s where C2_s >= 1e-15, else 0)
//     dp_i = -(1/p_i) (sum_c U_ic Y_ic + sum_j (X_ij + X_ji))   X = V o C (square) or W o log C, W = V o C (KL; W = 0 gives 0)
//
// k_fgw_bwd_full: one workgroup (4 wavefronts) per coupling (b, s), grid B*K.  T_s is read once.  dZ_s runs the exact arithmetic of k_fgw_bwd
// (a k-ordered fp32 fma chain per element, same variant choice), so its bits equal conan_fgw_barycenter_bwd's.  The two N^3 products
// A = H T_s and G_s = T_s^T A run on v_mfma_f32_16x16x4_f32 (exact fp32 fma chains) over 16 x 16 output tiles, dealt round-robin to the
// wavefronts.  Every operand is read as [k][16 consecutive columns] (H is staged transposed), so the four k rows of one MFMA hit distinct
// LDS banks for every pitch used here.  LDS = true: T_s, H^T and A at pitch P = roundup(N, 16) in LDS (3 P^2 floats, up to N = 112);
// else T_s is read from global memory and H^T / A go through a per-coupling scratch (2 N^2 floats, L2-resident), as the large coupling
// kernel does.  The dlam partials are written per coupling to part[B*K] and summed over b in a fixed order by k_fgw_grad_lam: no atomics,
// two passes are bit-identical.  dp is formed by the s = 0 workgroup of each molecule.
#include "common.h"

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int GR_NT = 256;          // 4 wavefronts
constexpr int GR_NW = GR_NT / 64;

struct FgwGradArgs {
    const float *T, *Ys, *Cs, *Y, *C, *dY, *dC, *p, *lambdas;
    float *dYs, *dCs, *dp, *part, *scratch;
    int K, N, d, loss, feat, strc, dys_lds;       // feat: feature term on (dY, !fixed_features); strc: structure products wanted
    int feat_p, strc_p;                           // dp terms
};

__device__ __forceinline__ float gr_pinv(const float *pb, int i, int N) {
    return pb ? (pb[i] > 0.f ? 1.0f / pb[i] : 0.f) : (float)N;      // massless node: no gradient (as k_fgw_bwd)
}

// D[i0.., j0..] += sum_k X[k][i] Yk[k][j] for one 16 x 16 tile: X, Yk row-major with pitch ld, N valid rows / columns (zero beyond).
__device__ __forceinline__ f32x4 gr_tile(const float *X, const float *Yk, int ld, int N, int i0, int j0, int lane) {
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    const int ci = i0 + (lane & 15), cj = j0 + (lane & 15), kq = lane >> 4;
    const bool vi = ci < N, vj = cj < N;
    for (int k0 = 0; k0 < N; k0 += 4) {
        const int k = k0 + kq;
        const float a = (vi && k < N) ? X[k * ld + ci] : 0.f;
        const float b = (vj && k < N) ? Yk[k * ld + cj] : 0.f;
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc, 0, 0, 0);
    }
    return acc;
}

template <bool LDS>
__global__ void __launch_bounds__(GR_NT) k_fgw_bwd_full(FgwGradArgs g) {
    extern __shared__ float gr_smem[];
    const int K = g.K, N = g.N, d = g.d;
    const int cid = blockIdx.x, b = cid / K, s = cid - b * K;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const size_t NN = (size_t)N * N;
    const float *Tg = g.T + (size_t)cid * NN;
    const float *pb = g.p ? g.p + (size_t)b * N : nullptr;
    const float lam = g.lambdas ? g.lambdas[s] : 1.0f / (float)K;
    const int P = LDS ? ((N + 15) & ~15) : N;
    float *red = gr_smem;                                   // [GR_NW] wavefront partials
    float *pl = gr_smem + GR_NW;                            // [N] 1/p (guarded)
    float *Tl = pl + ((N + 3) & ~3);                        // LDS: [P][P] T_s, [P][P] H^T, [P][P] A
    const float *Tm = LDS ? Tl : Tg;
    float *Ht = LDS ? Tl + (size_t)P * P : g.scratch + (size_t)cid * 2 * NN;
    float *Am = LDS ? Tl + (size_t)2 * P * P : g.scratch + (size_t)cid * 2 * NN + NN;

    for (int i = tid; i < N; i += GR_NT) pl[i] = gr_pinv(pb, i, N);
    if (LDS)
        for (int t = tid; t < (int)NN; t += GR_NT) { const int i = t / N, j = t - i * N; Tl[i * P + j] = Tg[t]; }
    if (g.strc) {                                           // H^T[k][i] = H[i][k] = V_ik (o C_ik) / (p_i p_k)
        const float *V = g.dC + (size_t)b * NN, *Cb = g.C ? g.C + (size_t)b * NN : nullptr;
        for (int t = tid; t < (int)NN; t += GR_NT) {
            const int i = t / N, k = t - i * N;
            float v = V[t];
            if (g.loss) v *= Cb[t];
            Ht[k * P + i] = v * (gr_pinv(pb, i, N) * gr_pinv(pb, k, N));
        }
    }
    // LDS: dY[b] staged in the A region (free until the first product) when it fits, so the fma chains below read no global memory
    const bool u_lds = LDS && g.feat && (g.dYs || g.part) && N * d <= P * P;
    if (u_lds)
        for (int t = tid; t < N * d; t += GR_NT) Am[t] = g.dY[(size_t)b * N * d + t];
    if (!LDS) __threadfence_block();
    __syncthreads();

    float part = 0.f;
    // ---- dZ_s = lam_s T_s^T diag(1/p) U, and its share of dlam_s: the arithmetic of k_fgw_bwd
    if (g.feat && (g.dYs || g.part)) {
        const float *U = u_lds ? Am : g.dY + (size_t)b * N * d;
        const float *Z = g.Ys + (size_t)cid * N * d;
        for (int t = tid; t < N * d; t += GR_NT) {
            const int j = t / d, c = t - j * d;
            float a = 0.f;
            if (g.dys_lds) {
                for (int i = 0; i < N; ++i) { const float gv = pl[i] * U[i * d + c]; a += Tm[i * P + j] * gv; }
            } else {
                for (int i = 0; i < N; ++i) a += Tm[i * P + j] * pl[i] * U[i * d + c];
            }
            if (g.dYs) g.dYs[(size_t)cid * N * d + t] = lam * a;
            if (g.part) part += a * Z[t];
        }
    }
    // ---- G_s = T_s^T (H T_s) on fp32 MFMA; dC2_s and the structure share of dlam_s from the accumulator tiles
    if (g.strc) {
        if (u_lds) __syncthreads();                         // every wavefront is done with the staged dY before A overwrites it
        const int nt = (N + 15) >> 4;
        for (int tile = wave; tile < nt * nt; tile += GR_NW) {
            const int i0 = (tile / nt) << 4, j0 = (tile % nt) << 4;
            const f32x4 acc = gr_tile(Ht, Tm, P, N, i0, j0, lane);
            const int col = j0 + (lane & 15);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = i0 + ((lane >> 4) << 2) + r;
                if (row < N && col < N) Am[row * P + col] = acc[r];
            }
        }
        if (!LDS) __threadfence_block();
        __syncthreads();
        const float *C2 = g.Cs + (size_t)cid * NN;
        float *dC2 = g.dCs ? g.dCs + (size_t)cid * NN : nullptr;
        for (int tile = wave; tile < nt * nt; tile += GR_NW) {
            const int i0 = (tile / nt) << 4, j0 = (tile % nt) << 4;
            const f32x4 acc = gr_tile(Tm, Am, P, N, i0, j0, lane);
            const int col = j0 + (lane & 15);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = i0 + ((lane >> 4) << 2) + r;
                if (row < N && col < N) {
                    const float gv = acc[r], c2 = C2[row * N + col];
                    float o;
                    if (g.loss == 0) {
                        o = lam * gv;
                        part += gv * c2;
                    } else {
                        o = c2 >= 1e-15f ? lam * gv / c2 : 0.f;             // torch.clamp(min=1e-15)'s backward mask
                        part += gv * logf(fmaxf(c2, 1e-15f));
                    }
                    if (dC2) dC2[row * N + col] = o;
                }
            }
        }
    }
    if (g.part) {                                           // fixed-order workgroup sum of the dlam_s partial
        part = wave_sum(part);
        if (lane == 0) red[wave] = part;
        __syncthreads();
        if (tid == 0) {
            float v = red[0];
            for (int w = 1; w < GR_NW; ++w) v += red[w];
            g.part[cid] = v;
        }
    }
    // ---- dp_i = -(1/p_i) (sum_c U_ic Y_ic + sum_j (X_ij + X_ji)): once per molecule
    if (g.dp && s == 0) {
        const float *U = g.dY + (size_t)b * N * d, *Yb = g.Y ? g.Y + (size_t)b * N * d : nullptr;
        const float *V = g.dC + (size_t)b * NN, *Cb = g.C ? g.C + (size_t)b * NN : nullptr;
        for (int i = tid; i < N; i += GR_NT) {
            float acc = 0.f;
            if (g.feat_p)
                for (int c = 0; c < d; ++c) acc += U[i * d + c] * Yb[i * d + c];
            if (g.strc_p) {
                for (int j = 0; j < N; ++j) {
                    const float cij = Cb[i * N + j], cji = Cb[j * N + i];
                    float xij = V[i * N + j] * cij, xji = V[j * N + i] * cji;
                    if (g.loss) {                                   // W o log C; an underflowed C (W = 0) contributes 0, not 0 * -inf
                        xij = xij != 0.f ? xij * logf(cij) : 0.f;
                        xji = xji != 0.f ? xji * logf(cji) : 0.f;
                    }
                    acc += xij + xji;
                }
            }
            const float pi = pb[i];
            g.dp[(size_t)b * N + i] = pi > 0.f ? -acc / pi : 0.f;
        }
    }
}

// dlam[s] = sum_b part[b*K + s], b ascending
__global__ void __launch_bounds__(64) k_fgw_grad_lam(const float *__restrict__ part, int B, int K, float *__restrict__ dlam) {
    const int s = blockIdx.x * 64 + threadIdx.x;
    if (s >= K) return;
    float v = 0.f;
    for (int b = 0; b < B; ++b) v += part[(size_t)b * K + s];
    dlam[s] = v;
}

constexpr size_t GR_LDS_MAX = 160 * 1024;

size_t gr_lds_bytes(int N, bool lds) {
    const size_t P = (size_t)((N + 15) & ~15);
    return (GR_NW + (size_t)((N + 3) & ~3) + (lds ? 3 * P * P : 0)) * sizeof(float);
}
bool gr_use_lds(int N) { return gr_lds_bytes(N, true) <= GR_LDS_MAX; }
size_t gr_al256(size_t v) { return (v + 255) & ~(size_t)255; }

}  // namespace

extern "C" {

long long conan_fgw_barycenter_bwd_full_workspace_bytes(int B, int K, int N, int d) {
    if (B <= 0 || K <= 0 || N <= 0 || d <= 0) return 0;
    size_t w = gr_al256((size_t)B * K * sizeof(float));
    if (!gr_use_lds(N)) w += (size_t)B * K * 2 * N * N * sizeof(float);
    return (long long)w;
}

int conan_fgw_barycenter_bwd_full(const float *T, const float *Ys, const float *Cs, const float *Y, const float *C, const float *dY,
                                  const float *dC, const float *p, const float *lambdas, int B, int K, int N, int d, int loss_fun,
                                  int fixed_structure, int fixed_features, float *dYs, float *dCs, float *dp, float *dlambdas,
                                  float *dinit_C, float *dinit_Y, void *workspace, void *stream) {
    if (!T || B <= 0 || K <= 0 || N <= 0 || d <= 0 || (loss_fun != 0 && loss_fun != 1)) return CONAN_E_BADARG;
    if ((dYs && fixed_features) || (dCs && fixed_structure) || (dinit_C && !fixed_structure) || (dinit_Y && !fixed_features))
        return CONAN_E_BADARG;                                  // gradients the update steps do not define
    if ((dCs && !Cs) || (dp && !p)) return CONAN_E_BADARG;
    const bool feat = dY && !fixed_features, strc_on = dC && !fixed_structure;
    if (dlambdas && ((feat && !Ys) || (strc_on && !Cs))) return CONAN_E_BADARG;
    if (dp && ((feat && !Y) || (strc_on && !C))) return CONAN_E_BADARG;
    if (strc_on && loss_fun == 1 && (dCs || dlambdas) && !C) return CONAN_E_BADARG;
    const bool lds = gr_use_lds(N);
    const bool strc = strc_on && (dCs || dlambdas);
    if ((dlambdas || (strc && !lds)) && !workspace) return CONAN_E_BADARG;
    hipStream_t st = as_stream(stream);
    const size_t NN = (size_t)N * N, Nd = (size_t)N * d;

    // the model path's request (dY only, dYs only): conan_fgw_barycenter_bwd itself
    if (!dCs && !dp && !dlambdas && !dinit_C && !dinit_Y && dYs && dY) return conan_fgw_barycenter_bwd(T, dY, p, lambdas, B, K, N, d, dYs, stream);

    if (dinit_C) {
        if (dC) (void)hipMemcpyAsync(dinit_C, dC, (size_t)B * NN * sizeof(float), hipMemcpyDeviceToDevice, st);
        else (void)hipMemsetAsync(dinit_C, 0, (size_t)B * NN * sizeof(float), st);
    }
    if (dinit_Y) {
        if (dY) (void)hipMemcpyAsync(dinit_Y, dY, (size_t)B * Nd * sizeof(float), hipMemcpyDeviceToDevice, st);
        else (void)hipMemsetAsync(dinit_Y, 0, (size_t)B * Nd * sizeof(float), st);
    }
    if (dYs && !feat) (void)hipMemsetAsync(dYs, 0, (size_t)B * K * Nd * sizeof(float), st);
    if (dCs && !strc_on) (void)hipMemsetAsync(dCs, 0, (size_t)B * K * NN * sizeof(float), st);
    const bool run = (dYs && feat) || (dCs && strc_on) || dlambdas || dp;
    if (run) {
        float *part = dlambdas ? static_cast<float *>(workspace) : nullptr;
        float *scratch = (strc && !lds) ? reinterpret_cast<float *>(static_cast<char *>(workspace) + gr_al256((size_t)B * K * sizeof(float)))
                                        : nullptr;
        FgwGradArgs a{T, Ys, Cs, Y, C, dY, dC, p, lambdas, feat ? dYs : nullptr, strc_on ? dCs : nullptr, dp, part, scratch,
                      K, N, d, loss_fun, feat ? 1 : 0, strc ? 1 : 0,
                      (((size_t)N * N + (size_t)N * d) * sizeof(float) <= 64 * 1024) ? 1 : 0,      // k_fgw_bwd's variant
                      (dp && feat) ? 1 : 0, (dp && strc_on) ? 1 : 0};
        const size_t lb = gr_lds_bytes(N, lds);
        if (lds) {
            (void)hipFuncSetAttribute(reinterpret_cast<const void *>(&k_fgw_bwd_full<true>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lb);
            k_fgw_bwd_full<true><<<B * K, GR_NT, lb, st>>>(a);
        } else {
            k_fgw_bwd_full<false><<<B * K, GR_NT, lb, st>>>(a);
        }
        CONAN_LAUNCH_CHECK();
        if (dlambdas) {
            k_fgw_grad_lam<<<(K + 63) / 64, 64, 0, st>>>(part, B, K, dlambdas);
            CONAN_LAUNCH_CHECK();
        }
    }
    return CONAN_OK;
}

}  // extern "C"
