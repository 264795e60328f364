// Two chained node-level Linear layers in ONE launch:
//
//     forward :  h = ssp(x W1^T + b1) ;  y  = h W2^T + b2 (+ residual)                 (InteractionBlock: conv.lin2 -> act -> lin, + x)
//     backward:  dh = (dy W2) * ssp'(h) ;  dx = dh W1                                   (the two input-gradient GEMMs and the activation
//                                                                                        derivative between them; h is the saved output)
//
// The same kernel with the activation moved behind the second layer serves the per-atom heads (lin1 -> lin2 -> act, schnet_no_sum.py:176-178,
// 225-231): forward  mid = x W1^T + b1 ;  y = ssp(mid W2^T + b2),  backward  g = dy * ssp'(y) (applied to the input rows and written out for
// the weight gradient) ; dmid = g W2 ; dx = dmid W1.  The two heads of the shared trunk (lin1 / lin2 and lin1_bary / lin2_bary) read the same x:
// k_mlp2_dual runs both in one launch each way and writes the sum of their input gradients once.
//
// At node level (25 k rows) a Linear launch is mostly fixed cost — 8.4 us of 13.5 us are weight staging, one tile per wave, the
// launch itself — and the layers of an interaction form a serial chain, so the only way to shorten it is to have fewer links.
// Mapping (as filter_fused.hip): the row index lives on the MFMA column (= lane), the channel on the MFMA row.  A wave owns one
// 32-row tile: GEMM1's B operand are its x rows straight from global memory (requested before the weights are staged), GEMM2's B
// operand IS GEMM1's accumulator after the element-wise step (register r of lane-half h = channel 32nb + (r&3) + 8(r>>2) + 4h, so
// the second weight is staged with the matching column permutation) — nothing crosses lanes or LDS between the two GEMMs.  Both
// products are two-plane fp16 splits on v_mfma_f32_32x32x16_f16 (fp32-class; fp_planes.h describes the form and its exact power-of-two
// scales: one per weight matrix, one per x row — and here one per row of the intermediate, taken from the accumulators).  Both weights
// (2 x 70 KB of planes) sit in LDS from the start: one staging phase, one barrier.  (The three-plane bf16 form of round 2
// needed 104 KB per weight and staged them one after the other with two more barriers.)  `mid`
// (h forward, dh backward) is also written out: the weight gradients of the two layers need it.
#include "fp_planes.h"

namespace {

constexpr int M2_THREADS = 256, M2_WAVES = 4;
constexpr int M2_NPL = 2;                                      // operand planes (two fp16 planes, fp_planes.h)

// Both weights are staged as WeightPlanes (fp_planes.h: fetch, then park), so that the global loads of BOTH can be in flight from the start
// of the kernel; the forward reads them as [n][k], the backward reads the forward weights transposed.  The second weight is parked with the
// column permutation m2_perm4: inside every group of 16 k's the columns are stored in the order in which a lane-half enumerates the accumulator
// registers of the previous GEMM (position 8h + j <-> (j&3) + 8(j>>2) + 4h); four consecutive, 4-aligned k's stay consecutive under that
// permutation, so the 8-byte stores survive it.
__device__ __forceinline__ int m2_perm4(int k) {
    const int a = (k & 15) >> 2;
    return (k & ~15) + 8 * (a & 1) + 4 * (a >> 1);
}
template <int NO, int KD, bool TRANS> using M2Planes = WeightPlanes<NO, KD, M2_THREADS, TRANS>;

// One wavefront's 32-row tile through both GEMMs and their element-wise steps, against the staged planes WB / WB2 (inverse scales unA / unB) and the
// biases BL [NA + NB]: everything of k_mlp2 behind the staging barrier.  xa / xb: the tile's input rows (MODE 3: already times ssp'), av: the saved
// activations of MODE 1.  SUM: what becomes of the finalised fp32 output — 0: stored to y; 1: kept in `keep`, nothing stored; 2: `keep` is added to it
// and the sum stored (k_mlp2_dual: the input gradient of two heads of one x, each addend finalised as on its own, written once).
template <int KA, int NA, int NB, int MODE, int SUM = 0>
__device__ __forceinline__ void m2_rows(const float4 (&xa)[KA / 16], const float4 (&xb)[KA / 16], const float4 (&av)[MODE == 1 ? NA / 32 : 1][4],
                                        const float *__restrict__ residual, const __bf16 *WB, const __bf16 *WB2, const float *BL, float unA, float unB,
                                        int m, int mr, bool valid, int h, int l31, float *__restrict__ mid_out, float *__restrict__ y,
                                        float4 (&keep)[SUM ? NB / 32 : 1][4]) {
    constexpr int SA = KA / 16, SB = NA / 16, MBA = NA / 32, MBB = NB / 32;
    constexpr int WSA = KA + 8, WSB = NA + 8;
    // ---------------- GEMM1^T: acc1[nb] = WA[32nb.., :] . x^T
    f32x16 acc1[MBA];
#pragma unroll
    for (int nb = 0; nb < MBA; ++nb)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc1[nb][r] = 0.f;
    float xsc, xu;
    pow2_scale(row_absmax<SA>(xa, xb), xsc, xu);
    const float un1 = xu * unA;                                // inverse of (row scale of x) x (scale of the first weight)
#pragma unroll
    for (int s = 0; s < SA; ++s) {
        f16x8 q1, q2;
        row_split(xa[s], xb[s], xsc, q1, q2);
        planes_kstep<NA, WSA>(WB, 16 * s + 8 * h, l31, q1, q2, acc1);
        __builtin_amdgcn_sched_barrier(0);
    }
#pragma unroll
    for (int nb = 0; nb < MBA; ++nb)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc1[nb][r] *= un1;
    // element-wise step on the accumulators (register r of half h is channel 32nb + (r&3) + 8(r>>2) + 4h) and the `mid` output
#pragma unroll
    for (int nb = 0; nb < MBA; ++nb)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            float v[4];
            if (MODE == 1) {
                const float a4[4] = {av[nb][q].x, av[nb][q].y, av[nb][q].z, av[nb][q].w};
#pragma unroll
                for (int u = 0; u < 4; ++u) v[u] = acc1[nb][4 * q + u] * (1.0f - 0.5f * __expf(-a4[u]));      // * ssp'(pre) from the saved output
            } else if (MODE == 3) {
#pragma unroll
                for (int u = 0; u < 4; ++u) v[u] = acc1[nb][4 * q + u];
            } else {
                const float4 bb = *reinterpret_cast<const float4 *>(&BL[32 * nb + 8 * q + 4 * h]);
                const float p4[4] = {acc1[nb][4 * q + 0] + bb.x, acc1[nb][4 * q + 1] + bb.y, acc1[nb][4 * q + 2] + bb.z, acc1[nb][4 * q + 3] + bb.w};
#pragma unroll
                for (int u = 0; u < 4; ++u) v[u] = MODE == 0 ? ssp_f(p4[u]) : p4[u];
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) acc1[nb][4 * q + u] = v[u];
            if (mid_out && valid)
                *reinterpret_cast<float4 *>(mid_out + (size_t)m * NA + 32 * nb + 8 * q + 4 * h) = make_float4(v[0], v[1], v[2], v[3]);
        }
    float4 rv[MODE == 0 ? MBB : 1][4];
    if (MODE == 0 && residual) {
        const float *rr = residual + (size_t)mr * NB + 4 * h;
#pragma unroll
        for (int nb = 0; nb < MBB; ++nb)
#pragma unroll
            for (int q = 0; q < 4; ++q) rv[nb][q] = *reinterpret_cast<const float4 *>(rr + 32 * nb + 8 * q);
    }

    // ---------------- GEMM2^T: acc2[nb] = WB[32nb.., :] . mid^T, B operand = acc1 (k order of the A fragments permuted to match)
    f32x16 acc2[MBB];
#pragma unroll
    for (int nb = 0; nb < MBB; ++nb)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc2[nb][r] = 0.f;
    float am = 0.f;                                            // the row of `mid`: 64 channels here, 64 on lane ^ 32
#pragma unroll
    for (int nb = 0; nb < MBA; ++nb)
#pragma unroll
        for (int r = 0; r < 16; ++r) am = fmaxf(am, fabsf(acc1[nb][r]));
    am = fmaxf(am, __shfl_xor(am, 32));
    float msc, mu;
    pow2_scale(am, msc, mu);
    const float un2 = mu * unB;
#pragma unroll
    for (int ms = 0; ms < SB; ++ms) {
        const int mb = ms >> 1, sgrp = ms & 1;
        float hv[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) hv[j] = acc1[mb][8 * sgrp + j];
        f16x8 q1, q2;
        split2h(hv, msc, q1, q2);
        planes_kstep<NB, WSB>(WB2, 32 * mb + 16 * sgrp + 8 * h, l31, q1, q2, acc2);
        __builtin_amdgcn_sched_barrier(0);
    }
    if (!valid) return;                                        // (no barrier behind this point)
#pragma unroll
    for (int nb = 0; nb < MBB; ++nb)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float4 bb = *reinterpret_cast<const float4 *>(&BL[NA + 32 * nb + 8 * q + 4 * h]);
            float4 o = make_float4(fmaf(acc2[nb][4 * q], un2, bb.x), fmaf(acc2[nb][4 * q + 1], un2, bb.y), fmaf(acc2[nb][4 * q + 2], un2, bb.z),
                                   fmaf(acc2[nb][4 * q + 3], un2, bb.w));
            if (MODE == 0 && residual) { o.x += rv[nb][q].x; o.y += rv[nb][q].y; o.z += rv[nb][q].z; o.w += rv[nb][q].w; }
            if (MODE == 2) { o.x = ssp_f(o.x); o.y = ssp_f(o.y); o.z = ssp_f(o.z); o.w = ssp_f(o.w); }
            if (SUM == 1) { keep[nb][q] = o; continue; }
            if (SUM == 2) { o.x += keep[nb][q].x; o.y += keep[nb][q].y; o.z += keep[nb][q].z; o.w += keep[nb][q].w; }
            *reinterpret_cast<float4 *>(y + (size_t)m * NB + 32 * nb + 8 * q + 4 * h) = o;
        }
}

// MODE 3: g = dy * ssp'(pre) from the saved output (ya / yb), in place and out for the weight gradient
template <int KA>
__device__ __forceinline__ void m2_ssp_bwd_row(float4 (&xa)[KA / 16], float4 (&xb)[KA / 16], const float4 (&ya)[KA / 16], const float4 (&yb)[KA / 16],
                                               float *__restrict__ in_out, int m, int h, bool valid) {
#pragma unroll
    for (int s = 0; s < KA / 16; ++s) {
        xa[s].x *= 1.0f - 0.5f * __expf(-ya[s].x); xa[s].y *= 1.0f - 0.5f * __expf(-ya[s].y);
        xa[s].z *= 1.0f - 0.5f * __expf(-ya[s].z); xa[s].w *= 1.0f - 0.5f * __expf(-ya[s].w);
        xb[s].x *= 1.0f - 0.5f * __expf(-yb[s].x); xb[s].y *= 1.0f - 0.5f * __expf(-yb[s].y);
        xb[s].z *= 1.0f - 0.5f * __expf(-yb[s].z); xb[s].w *= 1.0f - 0.5f * __expf(-yb[s].w);
        if (in_out && valid) {
            float *gr = in_out + (size_t)m * KA + 8 * h + 16 * s;
            *reinterpret_cast<float4 *>(gr) = xa[s];
            *reinterpret_cast<float4 *>(gr + 4) = xb[s];
        }
    }
}

// KA -> NA -> NB.  MODE 0: mid = ssp(acc1 + bA), y = acc2 + bB (+ residual).  MODE 1 (its backward): mid = acc1 * ssp'(aux) with aux the saved
// ssp output [M,NA], y = acc2; weights read transposed, no biases.  MODE 2: mid = acc1 + bA, y = ssp(acc2 + bB).  MODE 3 (its backward):
// the input rows are scaled by ssp'(aux), aux = the saved output [M,KA], and written to in_out; mid = acc1, y = acc2; transposed weights.
template <int KA, int NA, int NB, int MODE>
__global__ void __launch_bounds__(M2_THREADS) k_mlp2(const float *__restrict__ x, const float *__restrict__ wA, const float *__restrict__ bA,
                                                     const float *__restrict__ wB, const float *__restrict__ bB, const float *__restrict__ aux,
                                                     const float *__restrict__ residual, int M, float *__restrict__ mid_out, float *__restrict__ y,
                                                     float *__restrict__ in_out) {
    constexpr bool BWD = (MODE & 1) != 0;
    constexpr int SA = KA / 16, MBA = NA / 32;
    constexpr int WORDS_A = (M2_NPL * NA * (KA + 8)) / 2, WORDS_B = (M2_NPL * NB * (NA + 8)) / 2;
    constexpr int WORDS = WORDS_A + WORDS_B;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    __bf16 *WB = reinterpret_cast<__bf16 *>(lds);
    __bf16 *WB2 = reinterpret_cast<__bf16 *>(lds + WORDS_A);      // the second weight has its own buffer
    float *BL = lds + WORDS;                                   // [NA + NB] biases
    __shared__ float wred[2 * M2_WAVES];
    float unA = 1.0f, unB = 1.0f;                              // inverse plane scales of the two weights (fp16 form)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, h = lane >> 5;
    const int tile = blockIdx.x * M2_WAVES + wave;
    const int m = (tile << 5) + l31;
    const bool valid = m < M;
    const int mr = valid ? m : M - 1;

    // the wave's x rows and (backward) the saved activations are requested before any weight is staged
    float4 xa[SA], xb[SA];
    row_load<SA>(x, mr, KA, h, xa, xb);
    float4 av[MODE == 1 ? MBA : 1][4];
    if (MODE == 1) {
        const float *ar = aux + (size_t)mr * NA + 4 * h;
#pragma unroll
        for (int nb = 0; nb < MBA; ++nb)
#pragma unroll
            for (int q = 0; q < 4; ++q) av[nb][q] = *reinterpret_cast<const float4 *>(ar + 32 * nb + 8 * q);
    }
    float4 ya[SA], yb[SA];
    if (MODE == 3) row_load<SA>(aux, mr, KA, h, ya, yb);
    M2Planes<NA, KA, BWD> stA;
    M2Planes<NB, NA, BWD> stB;
    stA.fetch(wA);
    stB.fetch(wB);                                             // in flight during the first GEMM
    const float ma = wave_max(stA.absmax()), mb = wave_max(stB.absmax());
    if (lane == 0) { wred[wave] = ma; wred[M2_WAVES + wave] = mb; }
    __syncthreads();
    float a = wred[0], b = wred[M2_WAVES];
#pragma unroll
    for (int w = 1; w < M2_WAVES; ++w) { a = fmaxf(a, wred[w]); b = fmaxf(b, wred[M2_WAVES + w]); }
    float scA, scB;
    pow2_scale(a, scA, unA);
    pow2_scale(b, scB, unB);
    stA.park(WB, scA);
    stB.park(WB2, scB, [](int k) { return m2_perm4(k); });
    for (int t = tid; t < NA + NB; t += M2_THREADS) BL[t] = BWD ? 0.f : (t < NA ? bA[t] : bB[t - NA]);
    if (MODE == 3) m2_ssp_bwd_row<KA>(xa, xb, ya, yb, in_out, m, h, valid);
    __syncthreads();

    float4 none[1][4];
    m2_rows<KA, NA, NB, MODE>(xa, xb, av, residual, WB, WB2, BL, unA, unB, m, mr, valid, h, l31, mid_out, y, none);
}

// Two heads of ONE input in one launch — the per-atom heads lin1 / lin2 and lin1_bary / lin2_bary of the shared trunk.  Per head the arithmetic
// is k_mlp2's, bit for bit (own weight scales, own row scales, m2_rows).  MODE 2 (forward), one x for both; SPLIT: blockIdx.y is the head (one
// staging of one head's weights per workgroup), else a workgroup stages both heads' weights behind one pair of barriers and runs them one after
// the other on one load of its x rows.  MODE 3 (backward, never SPLIT): x / aux are per head (dy and the saved y); the input gradient of the
// first head stays in registers, finalised, and the second head's is added to it: dx = dx_a + dx_b, written once to hb.y.
// m_dev (nullable): device-side row count, rows beyond it are neither read nor written.
struct M2Head {
    const float *x, *wA, *bA, *wB, *bB, *aux;
    float *mid_out, *y, *in_out;
};
template <int KA, int NA, int NB, int MODE, bool SPLIT>
__global__ void __launch_bounds__(M2_THREADS) k_mlp2_dual(const M2Head ha, const M2Head hb, const int *__restrict__ m_dev, int M) {
    static_assert(MODE == 2 || (MODE == 3 && !SPLIT), "heads: lin1 -> lin2 -> act and its backward");
    constexpr bool BWD = MODE == 3;
    constexpr int NH = SPLIT ? 1 : 2, NX = BWD ? NH : 1;        // heads per workgroup, input row sets per wavefront
    constexpr int SA = KA / 16;
    constexpr int WORDS_A = (M2_NPL * NA * (KA + 8)) / 2, WORDS_B = (M2_NPL * NB * (NA + 8)) / 2;
    constexpr int WORDS = WORDS_A + WORDS_B;
    extern __shared__ __attribute__((aligned(16))) float lds[];           // NH x [planes of wA | planes of wB], then NH x [NA + NB] biases
    __shared__ float wred[NH * 2 * M2_WAVES];
    if (m_dev) M = min(M, *m_dev);
    if ((int)blockIdx.x * (32 * M2_WAVES) >= M) return;        // nothing to do for this workgroup (the same for all its threads; also M <= 0)
    const M2Head hd[2] = {SPLIT && blockIdx.y ? hb : ha, hb};
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int l31 = lane & 31, h = lane >> 5;
    const int m = ((blockIdx.x * M2_WAVES + wave) << 5) + l31;
    const bool valid = m < M;
    const int mr = valid ? m : M - 1;

    float4 xa[NX][SA], xb[NX][SA], ya[NX][SA], yb[NX][SA];
#pragma unroll
    for (int i = 0; i < NX; ++i) {
        row_load<SA>(hd[i].x, mr, KA, h, xa[i], xb[i]);
        if (BWD) row_load<SA>(hd[i].aux, mr, KA, h, ya[i], yb[i]);
    }
    M2Planes<NA, KA, BWD> stA[NH];
    M2Planes<NB, NA, BWD> stB[NH];
#pragma unroll
    for (int i = 0; i < NH; ++i) {
        stA[i].fetch(hd[i].wA);
        stB[i].fetch(hd[i].wB);
    }
#pragma unroll
    for (int i = 0; i < NH; ++i) {
        const float ma = wave_max(stA[i].absmax()), mb = wave_max(stB[i].absmax());
        if (lane == 0) { wred[(2 * i) * M2_WAVES + wave] = ma; wred[(2 * i + 1) * M2_WAVES + wave] = mb; }
    }
    __syncthreads();
    float unA[NH], unB[NH];
#pragma unroll
    for (int i = 0; i < NH; ++i) {
        float a = wred[(2 * i) * M2_WAVES], b = wred[(2 * i + 1) * M2_WAVES];
#pragma unroll
        for (int w = 1; w < M2_WAVES; ++w) { a = fmaxf(a, wred[(2 * i) * M2_WAVES + w]); b = fmaxf(b, wred[(2 * i + 1) * M2_WAVES + w]); }
        float scA, scB;
        pow2_scale(a, scA, unA[i]);
        pow2_scale(b, scB, unB[i]);
        stA[i].park(lds + i * WORDS, scA);
        stB[i].park(lds + i * WORDS + WORDS_A, scB, [](int k) { return m2_perm4(k); });
        float *BL = lds + NH * WORDS + i * (NA + NB);
        for (int t = tid; t < NA + NB; t += M2_THREADS) BL[t] = BWD ? 0.f : (t < NA ? hd[i].bA[t] : hd[i].bB[t - NA]);
        if (BWD) m2_ssp_bwd_row<KA>(xa[i], xb[i], ya[i], yb[i], hd[i].in_out, m, h, valid);
    }
    __syncthreads();

    float4 av[1][4];                                           // (MODE 1 only: unused here)
    float4 keep[BWD ? NB / 32 : 1][4];
#pragma unroll
    for (int i = 0; i < NH; ++i) {
        const __bf16 *WB = reinterpret_cast<const __bf16 *>(lds + i * WORDS), *WB2 = reinterpret_cast<const __bf16 *>(lds + i * WORDS + WORDS_A);
        const float *BL = lds + NH * WORDS + i * (NA + NB);
        if constexpr (!BWD) {
            float4 none[1][4];
            m2_rows<KA, NA, NB, MODE>(xa[0], xb[0], av, nullptr, WB, WB2, BL, unA[i], unB[i], m, mr, valid, h, l31, hd[i].mid_out, hd[i].y, none);
        } else if (i == 0) {
            m2_rows<KA, NA, NB, MODE, 1>(xa[i], xb[i], av, nullptr, WB, WB2, BL, unA[i], unB[i], m, mr, valid, h, l31, hd[i].mid_out, nullptr, keep);
        } else {
            m2_rows<KA, NA, NB, MODE, 2>(xa[i], xb[i], av, nullptr, WB, WB2, BL, unA[i], unB[i], m, mr, valid, h, l31, hd[i].mid_out, hd[i].y, keep);
        }
    }
}

template <int KA, int NA, int NB, int MODE>
int m2_launch(const float *x, const float *wA, const float *bA, const float *wB, const float *bB, const float *aux, const float *residual, int M,
              float *mid_out, float *y, float *in_out, hipStream_t s) {
    constexpr int WA = (M2_NPL * NA * (KA + 8)) / 2, WBw = (M2_NPL * NB * (NA + 8)) / 2;
    const size_t lds = ((size_t)(WA + WBw) + NA + NB) * 4;
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(&k_mlp2<KA, NA, NB, MODE>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    const int tiles = (M + 31) / 32;
    k_mlp2<KA, NA, NB, MODE><<<(tiles + M2_WAVES - 1) / M2_WAVES, M2_THREADS, lds, s>>>(x, wA, bA, wB, bB, aux, residual, M, mid_out, y, in_out);
    return hipGetLastError() == hipSuccess ? CONAN_OK : CONAN_E_LAUNCH;
}

template <int KA, int NA, int NB, int MODE, bool SPLIT>
int m2_launch_dual(const M2Head &ha, const M2Head &hb, const int *m_dev, int M, hipStream_t s) {
    constexpr int WA = (M2_NPL * NA * (KA + 8)) / 2, WBw = (M2_NPL * NB * (NA + 8)) / 2;
    const size_t lds = (SPLIT ? 1 : 2) * ((size_t)(WA + WBw) + NA + NB) * 4;
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(&k_mlp2_dual<KA, NA, NB, MODE, SPLIT>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    const int tiles = (M + 31) / 32;
    k_mlp2_dual<KA, NA, NB, MODE, SPLIT><<<dim3((tiles + M2_WAVES - 1) / M2_WAVES, SPLIT ? 2 : 1), M2_THREADS, lds, s>>>(ha, hb, m_dev, M);
    return hipGetLastError() == hipSuccess ? CONAN_OK : CONAN_E_LAUNCH;
}

}  // namespace

extern "C" {

int conan_mlp2_supported(int M, int K, int N1, int N2) { return (K == 128 && N1 == 128 && N2 == 128 && M >= 1 && M <= 65536) ? 1 : 0; }

int conan_mlp2_fwd(const float *x, const float *w1, const float *b1, const float *w2, const float *b2, const float *residual, int M, int K, int N1,
                   int N2, float *mid_out, float *y, void *stream) {
    if (!x || !w1 || !b1 || !w2 || !b2 || !y || M < 0) return CONAN_E_BADARG;
    if (M == 0) return CONAN_OK;
    if (!conan_mlp2_supported(M, K, N1, N2)) return CONAN_E_UNSUPPORTED;
    return m2_launch<128, 128, 128, 0>(x, w1, b1, w2, b2, nullptr, residual, M, mid_out, y, nullptr, as_stream(stream));
}

int conan_mlp2_bwd(const float *dy, const float *w2, const float *w1, const float *mid, int M, int K, int N1, int N2, float *dmid_out, float *dx,
                   void *stream) {
    if (!dy || !w1 || !w2 || !mid || !dx || M < 0) return CONAN_E_BADARG;
    if (M == 0) return CONAN_OK;
    if (!conan_mlp2_supported(M, K, N1, N2)) return CONAN_E_UNSUPPORTED;
    // dy [M,N2] -> (W2 read as [N2][N1]: contraction over n2) -> dmid [M,N1] -> (W1 read as [N1][K]) -> dx [M,K]
    return m2_launch<128, 128, 128, 1>(dy, w2, nullptr, w1, nullptr, mid, nullptr, M, dmid_out, dx, nullptr, as_stream(stream));
}

int conan_mlp2_outact_supported(int M, int K, int N1, int N2) { return (K == 128 && N1 == 64 && N2 == 64 && M >= 1 && M <= 65536) ? 1 : 0; }

int conan_mlp2_outact_fwd(const float *x, const float *w1, const float *b1, const float *w2, const float *b2, int M, int K, int N1, int N2,
                          float *mid_out, float *y, void *stream) {
    if (!x || !w1 || !b1 || !w2 || !b2 || !y || M < 0) return CONAN_E_BADARG;
    if (M == 0) return CONAN_OK;
    if (!conan_mlp2_outact_supported(M, K, N1, N2)) return CONAN_E_UNSUPPORTED;
    return m2_launch<128, 64, 64, 2>(x, w1, b1, w2, b2, nullptr, nullptr, M, mid_out, y, nullptr, as_stream(stream));
}

int conan_mlp2_outact_bwd(const float *dy, const float *y, const float *w2, const float *w1, int M, int K, int N1, int N2, float *g_out,
                          float *dmid_out, float *dx, void *stream) {
    if (!dy || !y || !w1 || !w2 || !dx || M < 0) return CONAN_E_BADARG;
    if (M == 0) return CONAN_OK;
    if (!conan_mlp2_outact_supported(M, K, N1, N2)) return CONAN_E_UNSUPPORTED;
    // g = dy * ssp'(y) [M,N2] -> (W2 read as [N2][N1]) -> dmid [M,N1] -> (W1 read as [N1][K]) -> dx [M,K]
    return m2_launch<64, 64, 128, 3>(dy, w2, nullptr, w1, nullptr, y, nullptr, M, dmid_out, dx, g_out, as_stream(stream));
}

int conan_mlp2_outact_dual_fwd(const float *x, const float *w1a, const float *b1a, const float *w2a, const float *b2a, const float *w1b, const float *b1b,
                               const float *w2b, const float *b2b, int M, int K, int N1, int N2, const int *m_dev, int form, float *mid_a, float *y_a,
                               float *mid_b, float *y_b, void *stream) {
    if (!x || !w1a || !b1a || !w2a || !b2a || !w1b || !b1b || !w2b || !b2b || !y_a || !y_b || M < 0 || (form != 0 && form != 1)) return CONAN_E_BADARG;
    if (M == 0) return CONAN_OK;
    if (!conan_mlp2_outact_supported(M, K, N1, N2)) return CONAN_E_UNSUPPORTED;
    const M2Head ha = {x, w1a, b1a, w2a, b2a, nullptr, mid_a, y_a, nullptr}, hb = {x, w1b, b1b, w2b, b2b, nullptr, mid_b, y_b, nullptr};
    return form == 0 ? m2_launch_dual<128, 64, 64, 2, true>(ha, hb, m_dev, M, as_stream(stream))
                     : m2_launch_dual<128, 64, 64, 2, false>(ha, hb, m_dev, M, as_stream(stream));
}

int conan_mlp2_outact_dual_bwd(const float *dy_a, const float *y_a, const float *w2a, const float *w1a, const float *dy_b, const float *y_b,
                               const float *w2b, const float *w1b, int M, int K, int N1, int N2, const int *m_dev, float *g_a, float *dmid_a, float *g_b,
                               float *dmid_b, float *dx, void *stream) {
    if (!dy_a || !y_a || !w1a || !w2a || !dy_b || !y_b || !w1b || !w2b || !dx || M < 0) return CONAN_E_BADARG;
    if (M == 0) return CONAN_OK;
    if (!conan_mlp2_outact_supported(M, K, N1, N2)) return CONAN_E_UNSUPPORTED;
    const M2Head ha = {dy_a, w2a, nullptr, w1a, nullptr, y_a, dmid_a, nullptr, g_a}, hb = {dy_b, w2b, nullptr, w1b, nullptr, y_b, dmid_b, dx, g_b};
    return m2_launch_dual<64, 64, 128, 3, false>(ha, hb, m_dev, M, as_stream(stream));
}

}  // extern "C"
