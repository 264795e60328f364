// What the ViSNet forward kernels (visnet.hip) and their gradients (visnet_bwd.hip) share: the backward differentiates exactly the
// forward's SiLU and cutoff, and both walk the edges with the same per-lane row accessors, run lengths and — stated once, below — edge walk.
#pragma once
#include <type_traits>
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

struct Vec3 { float x, y, z; };      // a unit vector d_ij: staged and handed out as one value
__device__ __forceinline__ Vec3 ld_vec3(const float *__restrict__ p, size_t e) { return {p[e * 3], p[e * 3 + 1], p[e * 3 + 2]}; }

#ifndef CONAN_V_EB
#define CONAN_V_EB 4
#endif
#ifndef CONAN_VB_RUN
#define CONAN_VB_RUN 16
#endif
constexpr bool V_HALF = true;         // H = 128: a half-wavefront per edge (32 lanes x float4 = one 512-byte row), two edges per instruction
constexpr int V_EB = CONAN_V_EB;      // edges in flight per wavefront
constexpr int V_RUN = CONAN_VB_RUN;   // edges per wavefront in the kernels that walk runs of consecutive edges (64 left too few wavefronts in flight)

// ---------------------------------------------------------------------------------------------- the edge walk
// Every edge kernel of visnet.hip / visnet_bwd.hip deals a list of edges to a wavefront in chunks: a run of V_RUN consecutive edges (walk_runs), a
// by-target CSR row (walk_row) or a by-source list through t_eid (walk_sources), the last two in chunks of 64.  Per chunk each lane STAGES one edge
// (its indices and whatever scalar hangs off it: cutoff, unit vector), guarded by lane < cnt; then the chunk's slots are taken V_EB at a time: the rows
// of all V_EB slots are requested (`load`) before the first is used (`use`), each slot getting its edge's staged values by cross-lane reads.  A
// kernel supplies stage / load / use and its epilogue; the three rules live here:
//  1. a staged value is handed out under a full EXEC mask, ahead of the live-slot test: never inside a conditional arm (the lane a cross-lane
//     read takes from must be active, and with HALF the two halves of a wavefront part ways at that test);
//  2. every loop around a hand-out has a lane-independent trip count (cnt and the chunk bounds are wave-uniform);
//  3. a slot past the end of the list reloads the list's last edge (min(slot, cnt - 1)) and is not used; live slots are used in list order, so a
//     sum over a list has a fixed order and is bitwise reproducible (HALF: even slots in lanes 0-31, odd ones in 32-63, folded once by vfold).
// Five kernels are written on it: k_ne_scale, k_attn_msg, k_edge_embed_bwd_x, k_attn_bwd_source, k_vec_aggregate_bwd_s.  Eight still carry their
// own copy of the skeleton.  k_vec_aggregate, k_edge_update, k_edge_update_bwd_t / _s, k_attn_bwd_target and k_vec_aggregate_bwd_v: their sums of
// products are contracted to fused multiply-adds by the compiler, which picked other contractions once the body sat in a lambda (last bits
// differ from the commit before the walk); they move here after their contractions are written out as explicit fmaf.  k_edge_embed and
// k_edge_embed_bwd_p: same bits on walk_runs, but 16 % more instructions and 2 % more time per launch (profiles/README.md).
template <int CPL_, bool HALF_>
struct EdgeLanes {
    static constexpr int CPL = CPL_, ES = HALF_ ? 2 : 1, SPAN = (HALF_ ? 32 : 64) * CPL_;      // channels per lane, edges per step, channels per pass
    int lane, hf, ll, wave, nw;
    __device__ __forceinline__ EdgeLanes() {
        constexpr bool HALF = HALF_;
        lane = threadIdx.x & 63;
        hf = HALF ? lane >> 5 : 0, ll = HALF ? (lane & 31) : lane;      // HALF: a half-wavefront per edge (H = 32 CPL), two edges per step
        wave = __builtin_amdgcn_readfirstlane((int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6)), nw = (gridDim.x * blockDim.x) >> 6;
    }
};
// The CPL channels of a lane in the pass that starts at channel `first` (a `cp` loop in the kernel, or blockIdx.y blocks of whole heads in the attention
// kernels): idle lanes (c0 >= H) read column 0 and store nothing.
struct Chan { int c0, cl; bool on; };
template <class L> __device__ __forceinline__ Chan chan_pass(const L &l, int first, int H) { const int c0 = first + l.ll * L::CPL; return {c0, c0 < H ? c0 : 0, c0 < H}; }

struct NoStage {};                                // a list that needs nothing per edge but the edge id
template <class S> struct Staged { int e; S s; };      // this lane's edge of the chunk
template <class S>
__device__ __forceinline__ S hand_out(const S &mine, int from) {      // every 32-bit field of what lane `from` staged
    if constexpr (std::is_empty_v<S>) return S{};
    else {
        static_assert(std::is_trivially_copyable_v<S> && sizeof(S) % 4 == 0, "staged values are ints and floats");
        int w[sizeof(S) / 4];
        __builtin_memcpy(w, &mine, sizeof(S));
#pragma unroll
        for (unsigned u = 0; u < sizeof(S) / 4; ++u) w[u] = __shfl(w[u], from, 64);
        S r;
        __builtin_memcpy(&r, w, sizeof(S));
        return r;
    }
}
// One chunk of cnt <= 64 list positions from `base`.  eid == nullptr: a position is an edge id; otherwise the edge id is eid[position].
// stage(e) -> S;  load(e, S) -> R, the rows of one slot;  use(e, S, R &), the arithmetic of a live slot.
template <class L, class Stage>
__device__ __forceinline__ auto stage_chunk(const L &l, int base, int cnt, const int *__restrict__ eid, Stage &&stage) {
    using S = decltype(stage(0));
    const int e = l.lane < cnt ? (eid ? eid[base + l.lane] : base + l.lane) : 0;
    return Staged<S>{e, l.lane < cnt ? stage(e) : S{}};
}
template <class L, class S, class Load, class Use>
__device__ __forceinline__ void chunk_slots(const L &l, int base, int cnt, bool by_eid, const Staged<S> &mine, Load &&load, Use &&use) {
    using R = decltype(load((size_t)0, mine.s));
    for (int t = 0; t < cnt; t += L::ES * V_EB) {
        R rows[V_EB];
#pragma unroll
        for (int b = 0; b < V_EB; ++b) {
            const int tt = min(t + L::ES * b + l.hf, cnt - 1);
            rows[b] = load(by_eid ? (size_t)__shfl(mine.e, tt, 64) : (size_t)(base + tt), hand_out(mine.s, tt));
        }
#pragma unroll
        for (int b = 0; b < V_EB; ++b) {
            const int slot = t + L::ES * b + l.hf, tt = min(slot, cnt - 1);
            const size_t e = by_eid ? (size_t)__shfl(mine.e, tt, 64) : (size_t)(base + slot);
            const S s = hand_out(mine.s, tt);      // before the halves diverge
            if (slot >= cnt) continue;
            use(e, s, rows[b]);
        }
    }
}
template <class L, class Stage, class Load, class Use>
__device__ __forceinline__ void walk_list(const L &l, int first, int last, const int *__restrict__ eid, Stage &&stage, Load &&load, Use &&use) {
    for (int base = first; base < last; base += 64) {
        const int cnt = min(64, last - base);
        chunk_slots(l, base, cnt, eid != nullptr, stage_chunk(l, base, cnt, eid, stage), load, use);
    }
}
// the by-target CSR row of node i: edge ids rowptr[i] .. rowptr[i + 1] - 1
template <class L, class Stage, class Load, class Use>
__device__ __forceinline__ void walk_row(const L &l, const int *__restrict__ rowptr, int i, Stage &&stage, Load &&load, Use &&use) {
    walk_list(l, rowptr[i], rowptr[i + 1], nullptr, stage, load, use);
}
// the by-source list of node j: edge ids t_eid[t_rowptr[j] .. t_rowptr[j + 1] - 1]
template <class L, class Stage, class Load, class Use>
__device__ __forceinline__ void walk_sources(const L &l, const int *__restrict__ t_rowptr, const int *__restrict__ t_eid, int j, Stage &&stage, Load &&load, Use &&use) {
    walk_list(l, t_rowptr[j], t_rowptr[j + 1], t_eid, stage, load, use);
}
// all E edges in runs of V_RUN consecutive ones, a run per wavefront, every channel pass of a run on the same staged values: load(c, e, S), use(c, e, S, R &)
template <class L, class Stage, class Load, class Use>
__device__ __forceinline__ void walk_runs(const L &l, int E, int H, Stage &&stage, Load &&load, Use &&use) {
    for (int base = l.wave * V_RUN; base < E; base += l.nw * V_RUN) {
        const int cnt = min(V_RUN, E - base);
        const auto mine = stage_chunk(l, base, cnt, nullptr, stage);
        for (int cp = 0; cp < H; cp += L::SPAN) {
            const Chan c = chan_pass(l, cp, H);
            chunk_slots(l, base, cnt, false, mine, [&](size_t e, const auto &s) { return load(c, e, s); }, [&](size_t e, const auto &s, auto &r) { use(c, e, s, r); });
        }
    }
}

// ---------------------------------------------------------------------------------------------- host side
inline int nblk(long long n) { long long b = (n + 255) / 256; return (int)(b < 1 ? 1 : (b > 4096 ? 4096 : b)); }
inline int edge_grid(int max_edges) { return nblk((long long)max_edges * (64 / V_RUN)); }      // a wavefront per run of V_RUN edges
inline int node_grid(int n) { return nblk((long long)n * 64); }                                 // a wavefront per node

// the instantiation <CPL, HALF> of an edge kernel at width H: f(std::integral_constant<int, CPL>, std::bool_constant<HALF>)
template <class F>
inline void with_width(int H, F &&f) {
    if (H == 128 && V_HALF) f(std::integral_constant<int, 4>{}, std::true_type{});
    else if (H % 128 == 0) f(std::integral_constant<int, 2>{}, std::false_type{});
    else f(std::integral_constant<int, 1>{}, std::false_type{});
}
// The attention kernels' own rule, for the forward and the backward entry point.  H a multiple of 128 (the classification backbone's 512, common.py:444-446):
// blocks of 128 channels on blockIdx.y, each a half-wavefront per edge — heads must not straddle a block (hd divides 128) and span a power-of-two
// number of 4-channel lanes.  Otherwise H <= 64 (<1>) or H == 128 (<2>), a head spanning lph lanes.
struct AttnShape { int rc; bool blocks128; int cpl, lph; };
inline AttnShape attn_shape(int H, int num_heads) {
    const int hd = H / num_heads;
    const bool blocks128 = H % 128 == 0 && V_HALF && hd % 4 == 0 && (((hd / 4) & (hd / 4 - 1)) == 0) && 128 % hd == 0;
    const int cpl = H > 64 ? (H + 63) / 64 : 1;
    if (!blocks128 && (H > 128 || (H > 64 && H != 128) || hd % cpl != 0)) return {CONAN_E_UNSUPPORTED, false, 0, 0};
    const int lph = blocks128 ? hd / 4 : hd / cpl;
    return {(lph & (lph - 1)) ? CONAN_E_UNSUPPORTED : CONAN_OK, blocks128, cpl, lph};
}
template <class F>
inline void with_attn_width(const AttnShape &a, int n, int H, F &&f) {      // f(CPL, HALF, grid)
    if (a.blocks128) f(std::integral_constant<int, 4>{}, std::true_type{}, dim3(node_grid(n), H / 128));
    else if (a.cpl == 2) f(std::integral_constant<int, 2>{}, std::false_type{}, dim3(node_grid(n)));
    else f(std::integral_constant<int, 1>{}, std::false_type{}, dim3(node_grid(n)));
}

}  // namespace

#define V_CHECK(cond) if (!(cond)) return CONAN_E_BADARG
