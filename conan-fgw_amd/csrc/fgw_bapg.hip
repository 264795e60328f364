// Coupling solve of fgw_barycenters(..., solver="BAPG") for gfx950: the reference's fgw_bregman (bregman.py:170-279; marginal_loss=False,
// symmetric), called for every input graph in every outer iteration (barycenter.py:118-160) with the outer max_iter and tol = 1e-4.
//
// One workgroup per (molecule b, input graph s), grid B*K; it takes the place of k_fgw_coupling in the outer loop of fgw.hip and hands the
// update stage the same things (T, Ypart = T Z, Cpart = T h(C2) T^T).  One iteration of the solve is two Bregman half-steps
//
//     T <- T * exp(-df(T) / eps);  T <- diag(p / rowsum T) T          df(T) = -2 alpha hC1 T hC2^T + (1 - alpha) M
//     T <- T * exp(-df(T) / eps);  T <- T diag(q / colsum T)          (hC1 = C1; hC2 = 2 C2, or log(C2 + 1e-15) for kl_loss)
//
// and ||T - Tprev||_F is compared with the tol at cpt % 10 == 0.  There is no inner Sinkhorn: the two N^3 products per half-step (A = C1 T,
// G = A hC2^T on fp64 MFMA) are the whole cost.  The arithmetic is the reference's multiplicative form in fp64, so it underflows where the
// reference does: a row or column of the iterate whose sum is zero makes the next scaling 0/0 (the reference's NaN, after which it only
// warns).  The kernel computes the same NaN and raises flags bit 2 of info for the molecule.
//
// Matrices (pitch P): T, A and Mb = (1 - alpha) M in fp64, the previous iterate Tp in fp32 (only read by the error check: its rounding moves
// ||T - Tprev|| by ~1e-8 of ||T||, far below the tol).  28 bytes per entry: in LDS up to N = 64 (LDS = true), else in the coupling scratch
// of the general kernel's global mode (L2-resident).  C1 (fp64) and C2 (fp32) are read from global memory by the products, as in k_fgw_coupling.
//
// ASYM: symmetric=False / None (bregman.py:199-222): df(T) = -alpha (hC1 T hC2^T + hC1^T T hC2) + (1 - alpha) M.  The second product needs the
// iterate after the first is done, so G1 = A hC2^T waits in one more fp64 matrix G (36 bytes per entry: LDS up to N = 64, else a scratch of
// its own behind the regular workspace, conan_fgw_workspace_bytes); C1^T is read through the element-reader form of the product.  Bit 1
// of y_zero selects symmetric=None: torch.allclose(C1, C1^T, atol=1e-10) and the same for C2 (bregman.py:199-200), per coupling solve, and the
// symmetric form when both hold.
#include "fgw_common.h"

namespace {

constexpr int BAPG_NW = 8;

__host__ __device__ inline size_t bapg_vec_bytes(int N, int NW = BAPG_NW) { return (size_t)((5 + NW) * N + 16) * 8; }

// PAIR: the pair form (conan_fgw_pair_fwd with solver = 2: the reference's fgw_bregman(M, C1, C2, p, q), bregman.py:170-279), as in k_fgw_coupling: M is the
// caller's tensor, C1 the caller's structure widened into Cw, T0 = outer(p, q) or G0 through the warm-start branch, max_iter / tol the solve's own, the error of
// every check goes to pr.errs and info[b] = {iterations, 0, flags, symmetric decision taken}.  A node without mass (rectangular pairs are embedded with such
// nodes) never divides: its entries of T are zero by construction and its scaling factor is set to 0; flag bit 2 is raised only when a node WITH mass has a
// zero sum — the guard the barycenter form already has.  One body text (fgw_bapg_body.inc) compiled into both kernels, PAIR a constant of
// each: k_fgw_coupling_bapg keeps its symbols and its code (see k_fgw_coupling).
template <bool LDS, bool KL, int NW, bool ASYM = false>
__global__ void __launch_bounds__(64 * NW) k_fgw_coupling_bapg(
    const float *__restrict__ Ys, const float *__restrict__ Cs, const float *__restrict__ ps, const float *__restrict__ pb,
    FgwDims D, conan_fgw_params prm, int outer, int y_zero, const double *__restrict__ Cw, const double *__restrict__ Yw,
    const int *__restrict__ active, float *__restrict__ Tw, int *__restrict__ info, char *__restrict__ scratch, size_t scratch_stride,
    fgw_part_t *__restrict__ Ypart, fgw_part_t *__restrict__ Cpart) {
    constexpr bool PAIR = false;
    [[maybe_unused]] const FgwPair pr{};
#include "fgw_bapg_body.inc"
}

// The pair form.  Same arguments, read as in k_fgw_coupling_pair: Ys = M, Cs = C2, ps = q, pb = p, Cw = the widened C1, Tw = T (in: G0 when warm).
template <bool LDS, bool KL, int NW, bool ASYM>
__global__ void __launch_bounds__(64 * NW) k_fgw_coupling_bapg_pair(
    const float *__restrict__ Ys, const float *__restrict__ Cs, const float *__restrict__ ps, const float *__restrict__ pb,
    FgwDims D, conan_fgw_params prm, int outer, int y_zero, const double *__restrict__ Cw, const double *__restrict__ Yw,
    const int *__restrict__ active, float *__restrict__ Tw, int *__restrict__ info, char *__restrict__ scratch, size_t scratch_stride,
    fgw_part_t *__restrict__ Ypart, fgw_part_t *__restrict__ Cpart, FgwPair pr) {
    constexpr bool PAIR = true;
#include "fgw_bapg_body.inc"
}

constexpr size_t BAPG_LDS_LIMIT = 160 * 1024;

__host__ inline size_t bapg_asym_stride(size_t NP) { return (NP * 36 + 15) / 16 * 16; }

}  // namespace

size_t conan_fgw_bapg_lds(int N, bool asym) { return bapg_vec_bytes(N) + (size_t)N * fgw_pitch(N) * (asym ? 36 : 28); }

size_t conan_fgw_bapg_asym_scratch_bytes(int B, int K, int N) {
    return conan_fgw_bapg_lds(N, true) <= BAPG_LDS_LIMIT ? 0 : (size_t)B * K * bapg_asym_stride((size_t)N * fgw_pitch(N));
}

void conan_fgw_bapg_coupling(const FgwCall &c, int outer, int y_zero) {
    const FgwDims &D = c.D;
    const bool asym = c.symmetric != 1;
    const size_t full = conan_fgw_bapg_lds(D.N, asym);
    const bool lds = full <= BAPG_LDS_LIMIT;
    const size_t bytes = lds ? full : bapg_vec_bytes(D.N);
    char *scratch = c.scratch;
    size_t scratch_stride = c.scratch_stride;
    if (asym) {      // symmetric=None travels in bit 1 of y_zero; outside LDS the matrices sit in the asymmetric solve's own scratch
        y_zero |= c.symmetric < 0 ? 2 : 0;
        if (!lds) { scratch = c.asym_scratch; scratch_stride = bapg_asym_stride((size_t)D.N * D.P); }
    }
    with_flags([&](auto L, auto KL, auto AS) {
        launch_lds(k_fgw_coupling_bapg<L.value, KL.value, BAPG_NW, AS.value>, D.B * D.K, 64 * BAPG_NW, bytes, c.s, c.Ys, c.Cs, c.ps, c.p, D, c.prm,
                   outer, y_zero, c.Cw, c.Yw, c.active, c.T, c.info, scratch, scratch_stride, c.Ypart, c.Cpart);
    }, lds, c.prm.loss_fun != 0, asym);
}

size_t conan_fgw_bapg_pair_stride(int N, bool asym) {
    const size_t NP = (size_t)N * fgw_pitch(N);
    return conan_fgw_bapg_lds(N, asym) <= BAPG_LDS_LIMIT ? 0 : asym ? bapg_asym_stride(NP) : (NP * 28 + 15) / 16 * 16;
}

void conan_fgw_bapg_pair(const FgwPairCall &c) {
    const bool asym = c.symmetric != 1;
    const size_t full = conan_fgw_bapg_lds(c.D.N, asym);
    const bool lds = full <= BAPG_LDS_LIMIT;
    with_flags([&](auto L, auto KL, auto AS) {
        launch_lds(k_fgw_coupling_bapg_pair<L.value, KL.value, BAPG_NW, AS.value>, c.D.B, 64 * BAPG_NW, lds ? full : bapg_vec_bytes(c.D.N), c.s, c.M, c.C2, c.q,
                   c.p, c.D, c.prm, c.warm, 1 | (c.symmetric < 0 ? 2 : 0), c.C1w, nullptr, nullptr, c.T, c.info, c.scratch, c.scratch_stride, nullptr, nullptr,
                   c.pr);
    }, lds, c.prm.loss_fun != 0, asym);
}
