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

}  // namespace
