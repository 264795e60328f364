// Split-precision operands of the MFMA kernels: the vector types, the plane splits and the power-of-two scales that a producer of planes
// and their consumer have to agree on bit for bit.  Every kernel that forms or reads planes takes them from here.
//
// Two-plane fp16 form: v = h1 + h2 up to 2^-22 |v| while the remainder v - h1 is a normal fp16 number (|v| >~ 0.06), and to 3e-8 absolute
// below that (fp16 subnormal spacing).  With the three products p1q1, p1q2, p2q1 (the dropped p2q2 is 2^-22 relative) an fp16 chain on
// v_mfma_f32_32x32x16_f16 reproduces the fp32 product to ~2.4e-7 at HALF the matrix-pipe time and ~2/3 of the splitting work of the
// three-plane bf16 form (6 products).  fp16's narrow exponent range (6e-5..65504) is met by exact power-of-two scales: a weight matrix by
// one factor (pow2_scale of its block maximum at staging time: max |w| in [256, 512), remainders normal, nothing near 65504), an x row by
// its own factor where rows vary (gemm_t.hip, mlp2.hip), a gradient tensor by grad_scale of its device-side maximum — each undone by one
// exact multiply where the accumulators are read.  Inside a scaled row or matrix, elements down to 2^-12 of the maximum keep 22 bits;
// below that the absolute error is 3e-8 / 256 of the maximum.
#pragma once
#include "common.h"

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));

// 8 floats exactly into three bf16 planes (six partial products per fp32 product on v_mfma_f32_32x32x16_bf16)
__device__ __forceinline__ void split3(const float *v, bf16x8 &p1, bf16x8 &p2, bf16x8 &p3) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const __bf16 h1 = (__bf16)v[j];
        const float r1 = v[j] - (float)h1;
        const __bf16 h2 = (__bf16)r1;
        const float r2 = r1 - (float)h2;
        p1[j] = h1; p2[j] = h2; p3[j] = (__bf16)r2;
    }
}
// 8 floats into two fp16 planes
__device__ __forceinline__ void split2h(const float *v, f16x8 &p1, f16x8 &p2) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const _Float16 h1 = (_Float16)v[j];
        p1[j] = h1; p2[j] = (_Float16)(v[j] - (float)h1);
    }
}
// ... of sc * v (sc an exact power of two)
__device__ __forceinline__ void split2h(const float *v, float sc, f16x8 &p1, f16x8 &p2) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const float t = v[j] * sc;
        const _Float16 h1 = (_Float16)t;
        p1[j] = h1; p2[j] = (_Float16)(t - (float)h1);
    }
}
// four consecutive k of row n of a two-plane image [2][N][WS] (16-bit elements): 8-byte stores, one per plane
__device__ __forceinline__ void store4_planes(void *planes, int N, int WS, int n, int k, const float *v4, float sc) {
    _Float16 *WH = reinterpret_cast<_Float16 *>(planes);
    f16x4 h1, h2;
#pragma unroll
    for (int e = 0; e < 4; ++e) { const float t = v4[e] * sc; h1[e] = (_Float16)t; h2[e] = (_Float16)(t - (float)h1[e]); }
    *reinterpret_cast<f16x4 *>(&WH[(0 * N + n) * WS + k]) = h1;
    *reinterpret_cast<f16x4 *>(&WH[(1 * N + n) * WS + k]) = h2;
}
// ... of a three-plane bf16 image [3][N][WS], unscaled
__device__ __forceinline__ void store4_planes3(void *planes, int N, int WS, int n, int k, const float *v4) {
    __bf16 *WB = reinterpret_cast<__bf16 *>(planes);
    bf16x4 q1, q2, q3;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        q1[j] = (__bf16)v4[j]; const float r1 = v4[j] - (float)q1[j];
        q2[j] = (__bf16)r1; q3[j] = (__bf16)(r1 - (float)q2[j]);
    }
    *reinterpret_cast<bf16x4 *>(&WB[(0 * N + n) * WS + k]) = q1;
    *reinterpret_cast<bf16x4 *>(&WB[(1 * N + n) * WS + k]) = q2;
    *reinterpret_cast<bf16x4 *>(&WB[(2 * N + n) * WS + k]) = q3;
}

__device__ __forceinline__ float absmax4(float m, const float4 &v) {
    return fmaxf(m, fmaxf(fmaxf(fabsf(v.x), fabsf(v.y)), fmaxf(fabsf(v.z), fabsf(v.w))));
}
// Maximum over the workgroup's NT threads, returned to every thread.  red: NT / 64 floats of LDS; the caller separates two uses of `red`
// by a barrier (there is none in front of the store here).
template <int NT>
__device__ __forceinline__ float block_absmax(float v, float *red) {
    v = wave_max(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    float m = red[0];
#pragma unroll
    for (int w = 1; w < NT / 64; ++w) m = fmaxf(m, red[w]);
    return m;
}

// The plane scale: sc = 2^k with amax * 2^k in [256, 512) and un = 2^-k, from the exponent field of amax.  Domain: exponent field 9..254
// (2^-118 <= amax < 2^128); outside it — zero, subnormal and tiny maxima, inf, NaN — both are 1.
__device__ __forceinline__ void pow2_scale(float amax, float &sc, float &un) {
    const int e = (int)((__float_as_uint(amax) >> 23) & 0xffu);
    const bool ok = e >= 9 && e <= 254;
    sc = ok ? __uint_as_float((unsigned)(262 - e) << 23) : 1.0f;
    un = ok ? __uint_as_float((unsigned)(e - 8) << 23) : 1.0f;
}
// The gradient scale: gsc = 2^k with gsc * gmax in [16, 32) and gun = 2^-k (1 / 1 for a zero or non-finite maximum).  `bound` is the
// caller's upper bound of what it forms from the scaled gradient at that nominal scale (filter backward: |s * dh1| <= 32 * F * max |w2|):
// above 16384 the scale is lowered until the bound fits fp16.  bound = 0: no such product.
__device__ __forceinline__ void grad_scale(float gmax, float bound, float &gsc, float &gun) {
    gsc = 1.0f; gun = 1.0f;
    if (gmax > 0.f && gmax < 3.0e38f) {
        int e; (void)frexpf(gmax, &e);
        int sh = 5 - e;
        if (bound > 16384.0f && bound < 3.0e38f) { int eb; (void)frexpf(bound * (1.0f / 16384.0f), &eb); sh -= eb; }
        gsc = ldexpf(1.0f, sh); gun = ldexpf(1.0f, -sh);
    }
}

// ---- a weight matrix as planes [.][NO][KD + 8] in LDS, staged by a workgroup of NT threads -------------------------------------------------
// The image is always [n][k]; the source is [NO][KD] (TRANS = false: a float4 is four consecutive k of one image row) or [KD][NO] (TRANS = true:
// the backward kernels read the forward weight transposed).  There a thread owns a 4(k) x 4(n) block: four float4 loads along n, transposed in
// registers (transpose4_row), 8-byte stores along k.  Inside a wavefront the blocks form a 4(k4) x 16(n4) patch with
// lane = (n4 & 3) | (k4 << 2) | ((n4 >> 2) << 4): every 16-lane group then covers 4 rows x 4 k-blocks = 16 distinct 8-byte bank slots (rows 4
// apart sit 64 B apart modulo the 256-B bank cycle).  fetch issues all of a thread's loads and consumes none, so that a kernel can have several
// weights and its first x rows in flight; absmax is the thread's share of the block maximum (block_absmax, pow2_scale); park splits and stores.
__device__ __forceinline__ void transpose4_row(const float4 *r, int e, float *v4) {      // v4[j] = element e of r[j]
#pragma unroll
    for (int j = 0; j < 4; ++j) v4[j] = e == 0 ? r[j].x : e == 1 ? r[j].y : e == 2 ? r[j].z : r[j].w;
}
template <int NO, int KD, int NT, bool TRANS>
struct WeightPlanes {
    static constexpr int V4 = NO * KD / 4, PER = (V4 + NT - 1) / NT;                                       // plain: float4s per thread
    static constexpr int PATCHES = (KD / 16) * (NO / 64), PERW = (PATCHES + NT / 64 - 1) / (NT / 64);      // transposed: 16(k) x 64(n) patches per wave
    float4 v[TRANS ? PERW * 4 : PER];
    // the block of slot u: image row n, first element k (transposed: of its four rows n .. n + 3); false: no such block
    static __device__ __forceinline__ bool block(int u, int &n, int &k) {
        const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
        if (!TRANS) {
            const int q = tid + u * NT;
            n = (4 * q) / KD; k = 4 * q - n * KD;
            return q < V4;
        }
        const int n4l = (lane & 3) | ((lane >> 4) << 2), k4l = (lane >> 2) & 3;
        const int pt = wave + u * (NT / 64);
        k = (pt / (NO / 64)) * 16 + 4 * k4l; n = (pt % (NO / 64)) * 64 + 4 * n4l;
        return pt < PATCHES;
    }
    __device__ __forceinline__ void fetch(const float *w, int ldw = TRANS ? NO : KD) {
#pragma unroll
        for (int u = 0; u < (TRANS ? PERW : PER); ++u) {
            int n, k;
            const bool ok = block(u, n, k);
#pragma unroll
            // plain: row n starts n * ldw floats in, written as 4 q + n * (ldw - KD) (n * KD + k = 4 q), which folds to 4 q for a dense
            // source.  Needs ldw >= KD (a row pitch is never below the row), or the difference would wrap through size_t.
            for (int j = 0; j < (TRANS ? 4 : 1); ++j) {
                const float *p = TRANS ? w + (size_t)(k + j) * ldw + n : w + (size_t)(n * KD + k) + (size_t)n * (ldw - KD);
                v[(TRANS ? 4 : 1) * u + j] = ok ? *reinterpret_cast<const float4 *>(p) : make_float4(0.f, 0.f, 0.f, 0.f);
            }
        }
    }
    __device__ __forceinline__ float absmax() const {
        float m = 0.f;
#pragma unroll
        for (int u = 0; u < (TRANS ? PERW * 4 : PER); ++u) m = absmax4(m, v[u]);
        return m;
    }
    // st(n, k, v4) for every run of four consecutive k of an image row that this thread holds
    template <class St>
    __device__ __forceinline__ void each4(St st) const {
#pragma unroll
        for (int u = 0; u < (TRANS ? PERW : PER); ++u) {
            int n, k;
            if (!block(u, n, k)) continue;
#pragma unroll
            for (int e = 0; e < (TRANS ? 4 : 1); ++e) {
                float v4[4];
                if (TRANS) transpose4_row(&v[4 * u], e, v4);
                else { v4[0] = v[u].x; v4[1] = v[u].y; v4[2] = v[u].z; v4[3] = v[u].w; }
                st(n + e, k, v4);
            }
        }
    }
    // two fp16 planes of sc * w; kperm: where the four k that start at k go (mlp2.hip stores its second weight in accumulator order)
    template <class P>
    __device__ __forceinline__ void park(void *planes, float sc, P kperm) const {
        each4([&](int n, int k, const float *v4) { store4_planes(planes, NO, KD + 8, n, kperm(k), v4, sc); });
    }
    __device__ __forceinline__ void park(void *planes, float sc) const { park(planes, sc, [](int k) { return k; }); }
};

// ---- a wavefront's 32 rows against staged planes: row m of x on lanes (m, h = 0 / 1), lane-half h holding k = 16 s + 8 h .. + 7 as xa[s], xb[s] --
template <int S>
__device__ __forceinline__ void row_load(const float *__restrict__ src, int row, int pitch, int h, float4 (&xa)[S], float4 (&xb)[S]) {
    const float *r = src + (size_t)row * pitch + 8 * h;
#pragma unroll
    for (int s = 0; s < S; ++s) {
        xa[s] = *reinterpret_cast<const float4 *>(r + 16 * s);
        xb[s] = *reinterpret_cast<const float4 *>(r + 16 * s + 4);
    }
}
template <int S>
__device__ __forceinline__ float row_absmax(const float4 (&xa)[S], const float4 (&xb)[S]) {
    float am = 0.f;
#pragma unroll
    for (int s = 0; s < S; ++s) { am = absmax4(am, xa[s]); am = absmax4(am, xb[s]); }
    return fmaxf(am, __shfl_xor(am, 32));                      // the other half of the row sits on lane ^ 32
}
// the B fragments of one k-step, xa[s] / xb[s] times sc as two fp16 planes.  (The loop over s stays with the caller: inside a function here the
// compiler vectorised the splits in another order and k_linear_t16<128, 128> went from 230 registers to 256 and scratch.)
__device__ __forceinline__ void row_split(const float4 &a, const float4 &b, float sc, f16x8 &q1, f16x8 &q2) {
    const float xv[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    split2h(xv, sc, q1, q2);
}
// one k-step: acc[nb] += W[32 nb + l31][colp .. colp + 7] x (q1 + q2) for the NB 32-feature blocks of an image [2][N][WS], as the three
// significant partial products (p2 q1, p1 q2, p1 q1: smallest first).  N and WS are template parameters: as run-time arguments the LDS
// addresses lost their no-wrap flags (inbounds nuw) and the address code of every caller changed.
template <int N, int WS, int NB>
__device__ __forceinline__ void planes_kstep(const void *planes, int colp, int l31, const f16x8 &q1, const f16x8 &q2, f32x16 (&acc)[NB]) {
    const _Float16 *WH = reinterpret_cast<const _Float16 *>(planes);
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
        const int row = 32 * nb + l31;
        const f16x8 p1 = *reinterpret_cast<const f16x8 *>(&WH[(0 * N + row) * WS + colp]);
        const f16x8 p2 = *reinterpret_cast<const f16x8 *>(&WH[(1 * N + row) * WS + colp]);
        acc[nb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(p2, q1, acc[nb], 0, 0, 0);
        acc[nb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(p1, q2, acc[nb], 0, 0, 0);
        acc[nb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(p1, q1, acc[nb], 0, 0, 0);
    }
}

}  // namespace
