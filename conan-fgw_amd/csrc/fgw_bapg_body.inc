// Body of k_fgw_coupling_bapg and k_fgw_coupling_bapg_pair (fgw_bapg.hip), compiled once into each: the kernel's arguments by name, the template parameters
// LDS, KL, NW, ASYM, and the constant PAIR and `FgwPair pr` that the including kernel defines.  Not a translation unit of its own.
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int NT = 64 * NW;
    [[maybe_unused]] int sym_auto = 0;
    if constexpr (ASYM) { sym_auto = y_zero >> 1; y_zero &= 1; }
    const int cid = blockIdx.x;
    const int b = cid / D.K, s = cid % D.K;
    if constexpr (!PAIR) { if (!fgw_active(active, D.B, b, outer)) return; }
    const int N = D.N, P = D.P, d = D.d;
    const int NN = N * N, NP = N * P;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);

    // ---- carve: [(5 + NW) N + 16] doubles of vectors, then the matrices (LDS or this coupling's scratch slice)
    double *pa = reinterpret_cast<double *>(smem), *qb = pa + N, *sc = pa + 2 * N, *y2a = pa + 3 * N, *z2a = pa + 4 * N;
    double *red = pa + 5 * N, *pm = red + 16;                  // pm[NW][N]: per-wavefront partial sums
    char *mats = LDS ? smem + bapg_vec_bytes(N, NW) : scratch + (size_t)cid * scratch_stride;
    double *T = reinterpret_cast<double *>(mats), *A = T + NP, *Mb = A + NP;
    [[maybe_unused]] double *G = Mb + NP;                      // ASYM only
    float *Tp = reinterpret_cast<float *>(ASYM ? G + NP : Mb + NP);

    const float *Z = Ys + ((size_t)b * D.K + s) * N * d;
    const float *C2 = Cs + ((size_t)b * D.K + s) * NN;
    const double *C1 = Cw + (size_t)b * NN;
    const double *Y = Yw + (size_t)b * N * d;
    float *Tg = Tw + ((size_t)b * D.K + s) * NN;
    const double alpha = (double)prm.alpha, eps = (double)prm.epsilon;

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
                for (int c = sub; c < d; c += LPI) {
                    const double yy = Y[i * d + c], zz = (double)Z[i * d + c];
                    y2 += yy * yy; z2 += zz * zz;
                }
#pragma unroll
            for (int o = 1; o < LPI; o <<= 1) { y2 += __shfl_xor(y2, o, 64); z2 += __shfl_xor(z2, o, 64); }
            if (i < N && sub == 0) { y2a[i] = y2; z2a[i] = z2; }
        }
    }
    [[maybe_unused]] bool asym = false;
    if constexpr (ASYM) {
        int nonsym = 0;
        if (sym_auto)
            for (int t = tid; t < NN; t += NT) {
                const int i = t / N, k = t - i * N;
                const double c1 = C1[i * N + k], c1t = C1[k * N + i], c2 = (double)C2[i * N + k], c2t = (double)C2[k * N + i];
                nonsym |= !(fabs(c1 - c1t) <= 1e-10 + 1e-5 * fabs(c1t)) || !(fabs(c2 - c2t) <= 1e-10 + 1e-5 * fabs(c2t));
            }
        asym = !sym_auto || __syncthreads_or(nonsym) != 0;              // (workgroup-uniform)
    }
    __syncthreads();
    // ---- T0: warm start from the previous outer iteration, else outer(p, q)      (bregman.py:197-198)
    for (int t = tid; t < NN; t += NT) {
        const int i = t / N, j = t - i * N;
        T[i * P + j] = (outer > 0 && prm.warmstart) ? (double)Tg[t] : pa[i] * qb[j];
        if constexpr (PAIR) { if (!(outer > 0 && prm.warmstart)) T[i * P + j] = (double)(float)(pa[i] * qb[j]); }      // the start a caller can pass as G0 (fp32), bit for bit
    }
    // ---- Mb = (1 - alpha) M,  M = clamp(|y_i|^2 + |z_j|^2 - 2 y_i.z_j, 0)    (utils.py:154-171)
    if (!y_zero) mm_f64_glb<NW, true>(N, N, d, Y, d, Z, d, [&](int i, int j, double v) { Mb[i * P + j] = v; });
    __syncthreads();
    for (int t = tid; t < NN; t += NT) {
        const int i = t / N, j = t - i * N;
        double m = -2.0 * (y_zero ? 0.0 : Mb[i * P + j]);
        m += y2a[i]; m += z2a[j];
        m = m > 0.0 ? m : 0.0;
        if constexpr (PAIR) m = (double)pr.M[(size_t)b * NN + t];     // the caller's cost, as given
        Mb[i * P + j] = (1.0 - alpha) * m;
    }
    __syncthreads();

    // T <- T * exp(-df(T) / eps) in place (the second product reads A, not T).  Entries of a massless row / column (fgw.py's embedding of
    // other sizes) stay exactly zero: the rectangular problem of the reference has no such entries.
    auto bregman_factor = [&]() {
        mm_f64_glb<NW, false>(N, N, N, C1, N, T, P, [&](int i, int j, double v) { A[i * P + j] = v; });      // A = C1 T
        __syncthreads();
        if constexpr (ASYM) {
            if (asym) {      // G = A hC2^T; A = C1^T T; T <- T exp(-(-alpha' (G + A hC2) + Mb) / eps)
                if constexpr (KL)
                    mm_f64<NW>(N, N, N, [&](int i, int k) { return A[i * P + k]; }, [&](int k, int j) { return log((double)C2[j * N + k] + 1e-15); },
                               [&](int i, int j, double g) { G[i * P + j] = g; });
                else
                    mm_f64_glb<NW, true>(N, N, N, A, P, C2, N, [&](int i, int j, double g) { G[i * P + j] = g; });
                __syncthreads();
                mm_f64<NW>(N, N, N, [&](int i, int k) { return C1[k * N + i]; }, [&](int k, int j) { return T[k * P + j]; },
                           [&](int i, int j, double v) { A[i * P + j] = v; });
                __syncthreads();
                auto upd2 = [&](int i, int j, double g) {      // square: hC2 = 2 C2 (factor 2 folded in)
                    const double x = T[i * P + j] * exp(-(-(KL ? 1.0 : 2.0) * alpha * (G[i * P + j] + g) + Mb[i * P + j]) / eps);
                    T[i * P + j] = (pa[i] > 0.0 && qb[j] > 0.0) ? x : 0.0;
                };
                if constexpr (KL)
                    mm_f64<NW>(N, N, N, [&](int i, int k) { return A[i * P + k]; }, [&](int k, int j) { return log((double)C2[k * N + j] + 1e-15); }, upd2);
                else
                    mm_f64_glb<NW, false>(N, N, N, A, P, C2, N, upd2);
                __syncthreads();
                return;
            }
        }
        auto upd = [&](int i, int j, double g) {        // g = (A hC2^T)_ij / c with c = 2 (square: hC2 = 2 C2, folded into the factor) or 1
            const double x = T[i * P + j] * exp(-(-(KL ? 2.0 : 4.0) * alpha * g + Mb[i * P + j]) / eps);
            T[i * P + j] = (pa[i] > 0.0 && qb[j] > 0.0) ? x : 0.0;
        };
        if constexpr (KL)
            mm_f64<NW>(N, N, N, [&](int i, int k) { return A[i * P + k]; }, [&](int k, int j) { return log((double)C2[j * N + k] + 1e-15); }, upd);
        else
            mm_f64_glb<NW, true>(N, N, N, A, P, C2, N, upd);
        __syncthreads();
    };

    int cpt = 0, zero_sum = 0;
    double err = 1e15;                                                  // bregman.py:240
    while (err > (double)prm.inner_tol && cpt < prm.max_iter) {
        const bool check = cpt % 10 == 0;
        if (check)
            for (int t = tid; t < NN; t += NT) { const int i = t / N, j = t - i * N; Tp[i * P + j] = (float)T[i * P + j]; }
        // ---- rows: T <- T exp(-df/eps); T <- diag(p / rowsum T) T
        bregman_factor();
        for (int i = lane; i < N; i += 64) {                            // lane <-> row, the wavefronts split the columns
            double rs = 0.0;
            for (int j = wave; j < N; j += NW) rs += T[i * P + j];
            pm[wave * N + i] = rs;
        }
        __syncthreads();
        for (int i = tid; i < N; i += NT) {
            double rs = 0.0;
#pragma unroll
            for (int w = 0; w < NW; ++w) rs += pm[w * N + i];
            if (pa[i] > 0.0 && !(rs > 0.0)) zero_sum = 1;
            sc[i] = pa[i] > 0.0 ? pa[i] / rs : 0.0;                     // p_i / 0: the reference's NaN (inf * 0) follows
        }
        __syncthreads();
        for (int t = tid; t < NN; t += NT) { const int i = t / N, j = t - i * N; T[i * P + j] *= sc[i]; }
        __syncthreads();
        // ---- columns: T <- T exp(-df/eps); T <- T diag(q / colsum T)
        bregman_factor();
        for (int j = lane; j < N; j += 64) {                            // lane <-> column, the wavefronts split the rows
            double cs = 0.0;
            for (int i = wave; i < N; i += NW) cs += T[i * P + j];
            pm[wave * N + j] = cs;
        }
        __syncthreads();
        for (int j = tid; j < N; j += NT) {
            double cs = 0.0;
#pragma unroll
            for (int w = 0; w < NW; ++w) cs += pm[w * N + j];
            if (qb[j] > 0.0 && !(cs > 0.0)) zero_sum = 1;
            sc[j] = qb[j] > 0.0 ? qb[j] / cs : 0.0;
        }
        __syncthreads();
        double e2 = 0.0;
        for (int t = tid; t < NN; t += NT) {
            const int i = t / N, j = t - i * N;
            const double x = T[i * P + j] * sc[j];
            T[i * P + j] = x;
            if (check) { const double df = x - (double)Tp[i * P + j]; e2 += df * df; }
        }
        if (check) {
            err = sqrt(block_sum_d<NW>(e2, red));                     // (NaN ends the loop, as in the reference)
            if constexpr (PAIR) { if (tid == 0) pr.errs[(size_t)b * pr.nerr + cpt / 10] = (float)err; }      // log["err"] (bregman.py:257-258)
        } else __syncthreads();
        ++cpt;
    }
    if constexpr (PAIR) {
        const int zero = __syncthreads_or(zero_sum);
        for (int t = tid; t < NN; t += NT) { const int i = t / N, j = t - i * N; Tg[t] = (float)T[i * P + j]; }
        int sym_taken = 1;
        if constexpr (ASYM) sym_taken = asym ? 0 : 1;
        if (tid == 0) { info[b * 4 + 0] = cpt; info[b * 4 + 1] = 0; info[b * 4 + 2] = zero ? 4 : 0; info[b * 4 + 3] = sym_taken; }
        return;
    }
    if (__syncthreads_or(zero_sum) && tid == 0) atomicOr(&info[b * 4 + 3], 4);
    for (int t = tid; t < NN; t += NT) { const int i = t / N, j = t - i * N; Tg[t] = (float)T[i * P + j]; }
    if (tid == 0) atomicAdd(&info[b * 4 + 1], cpt);                     // BAPG iterations (word 2, Sinkhorn iterations, stays 0)
    // ---- contributions to the barycenter update (summed over s by k_fgw_update_parts)
    if (!prm.fixed_features) {                                          // Ypart = T @ Z                      (utils.py:90-95)
        fgw_part_t *Yp = Ypart + ((size_t)b * D.K + s) * N * d;
        mm_f64_glb<NW, false>(N, d, N, T, P, Z, d, [&](int i, int c, double v) { Yp[(size_t)i * d + c] = (fgw_part_t)v; });
    }
    if (!prm.fixed_structure) {                                         // Cpart = T @ h(C2) @ T^T            (utils.py:67-87)
        fgw_part_t *Cp = Cpart + ((size_t)b * D.K + s) * NN;
        if constexpr (KL)
            mm_f64<NW>(N, N, N, [&](int i, int k) { return T[i * P + k]; },
                       [&](int k, int j) { const double cv = (double)C2[k * N + j]; return log(cv > 1e-15 ? cv : 1e-15); },
                       [&](int i, int j, double v) { A[i * P + j] = v; });
        else
            mm_f64_glb<NW, false>(N, N, N, T, P, C2, N, [&](int i, int j, double v) { A[i * P + j] = v; });
        __syncthreads();
        mm_f64_glb<NW, true>(N, N, N, A, P, T, P, [&](int i, int j, double v) { Cp[i * N + j] = (fgw_part_t)v; });
    }
