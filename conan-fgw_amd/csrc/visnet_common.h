// What the ViSNet forward kernels (visnet.hip) and their gradients (visnet_bwd.hip) share: the backward differentiates exactly the
// forward's SiLU and cutoff, and both walk the edges with the same per-lane row accessors and run lengths.
#pragma once
#include "common.h"

namespace {

__device__ __forceinline__ float sigmoid_f(float v) { return __builtin_amdgcn_rcpf(1.0f + __expf(-v)); }      // hardware reciprocal (1 ulp) instead of an IEEE division
__device__ __forceinline__ float silu_f(float v) { return v * sigmoid_f(v); }
__device__ __forceinline__ float dsilu_f(float v) { const float s = sigmoid_f(v); return s * (1.0f + v * (1.0f - s)); }
__device__ __forceinline__ float cos_cutoff(float d, float cutoff) {      // CosineCutoff, torch_geometric_visnet.py:33-46
    return d < cutoff ? 0.5f * (cosf(__fdiv_rn(d * 3.14159265358979323846f, cutoff)) + 1.0f) : 0.0f;
}

// CPL consecutive channels of one row as ONE load / store (float2 for CPL = 2: c0 is even and every row starts at a multiple of H floats from a
// 256-byte aligned allocation; the compiler cannot prove that and would issue two dword instructions)
template <int CPL>
__device__ __forceinline__ void vld(const float *__restrict__ p, float (&r)[CPL]) {
    if constexpr (CPL == 4) { const float4 t = *reinterpret_cast<const float4 *>(p); r[0] = t.x; r[1] = t.y; r[2] = t.z; r[3] = t.w; }
    else if constexpr (CPL == 2) { const float2 t = *reinterpret_cast<const float2 *>(p); r[0] = t.x; r[1] = t.y; }
    else {
#pragma unroll
        for (int u = 0; u < CPL; ++u) r[u] = p[u];
    }
}
template <int CPL, bool HALF>
__device__ __forceinline__ void vfold(float (&a)[CPL]) {      // HALF: even entries (lanes 0-31) + odd entries (lanes 32-63), fixed order
    if constexpr (HALF) {
#pragma unroll
        for (int u = 0; u < CPL; ++u) a[u] += __shfl_xor(a[u], 32, 64);
    }
}
template <int CPL>
__device__ __forceinline__ void vst(float *__restrict__ p, const float (&r)[CPL]) {
    if constexpr (CPL == 4) *reinterpret_cast<float4 *>(p) = make_float4(r[0], r[1], r[2], r[3]);
    else if constexpr (CPL == 2) *reinterpret_cast<float2 *>(p) = make_float2(r[0], r[1]);
    else {
#pragma unroll
        for (int u = 0; u < CPL; ++u) p[u] = r[u];
    }
}

#ifndef CONAN_V_EB
#define CONAN_V_EB 4
#endif
#ifndef CONAN_VB_RUN
#define CONAN_VB_RUN 16
#endif
constexpr bool V_HALF = true;         // H = 128: a half-wavefront per edge (32 lanes x float4 = one 512-byte row), two edges per instruction
constexpr int V_EB = CONAN_V_EB;      // edges in flight per wavefront
constexpr int V_RUN = CONAN_VB_RUN;   // edges per wavefront in the kernels that walk runs of consecutive edges (64 left too few wavefronts in flight)

inline int nblk(long long n) { long long b = (n + 255) / 256; return (int)(b < 1 ? 1 : (b > 4096 ? 4096 : b)); }

}  // namespace

#define V_CHECK(cond) if (!(cond)) return CONAN_E_BADARG
