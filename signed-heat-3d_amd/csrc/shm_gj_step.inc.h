// The body of gj_step_kernel (shm_kernels.hip.h, which includes this file once per mode and holds the description): SHM_GJ_STEP_NAME is the kernel's name,
// SHM_GJ_STEP_MODE 0 the Gauss-Jordan chain link (kGjStepInverse), 1 the elimination confined to the trailing matrix (kGjStepLdl), SHM_GJ_STEP_EXTRA_PARAM the
// latter's extra argument.  Two kernels of one text rather than a template or a shared inlined body: the Gauss-Jordan kernel keeps its name (the register test
// reads the compiler's report by it) and comes out of the compiler instruction for instruction as before the second mode existed (tools/device_code_diff.sh).
static __global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(SHM_GJ_STEP_WAVES, SHM_GJ_STEP_WAVES))) void SHM_GJ_STEP_NAME(
    double* __restrict__ G, int ld, int nb, int k, const double* __restrict__ Rp /* [64][ld] of step k-1 */, const double* __restrict__ Cp /* [ld][64] */,
    double* __restrict__ Rn, double* __restrict__ Cn, int* __restrict__ flag, int prio SHM_GJ_STEP_EXTRA_PARAM) {
    constexpr int MODE = SHM_GJ_STEP_MODE;

    __shared__ double smem[kGjStepLds];
    static_assert(kGjStepLds >= kGjUpdateLds && kGjStepScratch >= 8 * kGJ, "LDS carve");
    if (prio) __builtin_amdgcn_s_setprio(3);   // (see gj_panels_kernel)
    const int nN = MODE == kGjStepLdl ? shm::ldl_panel_count(nb, k) : (k < nb ? nb : 0);
    if ((int)blockIdx.x >= nN) {
#if SHM_GJ_STEP_MODE == 1
        const int nS = shm::ldl_store_count(nb, k);
        if ((int)blockIdx.x < nN + nS) {
            // ---- store role: L_b,k-1 = X_b = R_k-1[:, b]^T into tile (b, k-1), b >= k (nobody reads that tile again before the superblock inverses)
            double(*xt)[kGJ + 1] = reinterpret_cast<double(*)[kGJ + 1]>(smem);
            const size_t ob = (size_t)(k + (int)blockIdx.x - nN) * kGJ, oc = (size_t)(k - 1) * kGJ;
            for (int t = threadIdx.x; t < kGJ * kGJ; t += kBlock) {
                const int i = t / kGJ, j = t % kGJ;
                xt[i][j] = Rp[(size_t)i * ld + ob + j];
            }
            __syncthreads();
            for (int t = threadIdx.x; t < kGJ * kGJ; t += kBlock) {
                const int i = t / kGJ, j = t % kGJ;
                G[(ob + i) * ld + oc + j] = xt[j][i];
            }
            return;
        }
        {
            // ---- update role: step k-1 on the trailing tiles
            int ti, tj;
            shm::ldl_update_tile(k, blockIdx.x - (unsigned)(nN + nS), ti, tj);
            gj_update_tile(G, ld, ti, tj, -1, Rp, 0, Cp, kGJ, 0, kGJ, smem);
            return;
        }
#endif
        // ---- update role: step k-1 on every tile (bi >= bj) without a block index k
        int bi, bj;
        gj_tri_decode(blockIdx.x - (unsigned)nN, bi, bj);   // over nb - 1 blocks (k < nb) or all nb (last launch)
        if (k < nb) {
            if (bi >= k) bi += 1;
            if (bj >= k) bj += 1;
        }
        gj_update_tile(G, ld, bi, bj, k - 1, Rp, 0, Cp, kGJ, 0, kGJ, smem);
        return;
    }
    // ---- panel role
    double(*x)[kGJ + 1] = reinterpret_cast<double(*)[kGJ + 1]>(smem);
    double* scratch = smem + kGJ * (kGJ + 1);
    double(*prow)[kGJ + 1] = reinterpret_cast<double(*)[kGJ + 1]>(scratch);
#if SHM_GJ_STEP_MODE == 1
    const int b = k + (int)blockIdx.x;
#else
    const int b = blockIdx.x;
#endif
    const bool below = b >= k;
    const int bi = below ? b : k, bj = below ? k : b;   // the stored tile of the cross
    const size_t o = (size_t)k * kGJ, ob = (size_t)b * kGJ, oi = (size_t)bi * kGJ, oj = (size_t)bj * kGJ;
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, wr = w >> 1, wc = w & 1, l15 = lane & 15, l4 = lane >> 4;
    const int ty = threadIdx.x >> 4, tx = threadIdx.x & 15;
    double r[4][4];      // the pivot tile, thread (ty, tx) owning the 4 x 4 block (ty, tx)
    double* Cb = Cn + ob * kGJ;   // C_k[b], 64 x 64
    if (k > 0) {
        // accumulator layout: row = wr 32 + a 16 + l4 + 4 q, col = wc 32 + c 16 + l15.  Two products C[rows] R[:, cols], one after the other (together their
        // accumulators and operands do not fit the register cap), each in two groups of eight k-steps whose 32 operand loads are issued together, ahead of the
        // group's matrix instructions: left to itself the compiler waits for every k-step's loads before it issues the next ones -- 16 round trips to L2, a
        // quarter of this role's time.
        auto product = [&](gj_f64x4(&acc)[2][2], size_t orow, size_t ocol) {
#pragma unroll
            for (int a = 0; a < 2; a++)
#pragma unroll
                for (int c = 0; c < 2; c++) acc[a][c] = gj_f64x4{0., 0., 0., 0.};
#pragma unroll 1
            for (int g = 0; g < 2; g++) {
                double af[8][2], bf[8][2];
#pragma unroll
                for (int u = 0; u < 8; u++) {
                    const int kk = 32 * g + 4 * u + l4;
#pragma unroll
                    for (int a = 0; a < 2; a++) af[u][a] = Cp[(orow + wr * 32 + a * 16 + l15) * kGJ + kk];
#pragma unroll
                    for (int c = 0; c < 2; c++) bf[u][c] = Rp[(size_t)kk * ld + ocol + wc * 32 + c * 16 + l15];
                }
#pragma unroll
                for (int u = 0; u < 8; u++)
#pragma unroll
                    for (int a = 0; a < 2; a++)
#pragma unroll
                        for (int c = 0; c < 2; c++) acc[a][c] = __builtin_amdgcn_mfma_f64_16x16x4f64(af[u][a], bf[u][c], acc[a][c], 0, 0, 0);
            }
        };
        {
            gj_f64x4 accp[2][2];
            product(accp, o, o);   // the pivot tile: G[k, k] - C[k] R[:, k]
#pragma unroll
            for (int a = 0; a < 2; a++)
#pragma unroll
                for (int c = 0; c < 2; c++)
#pragma unroll
                    for (int q = 0; q < 4; q++) {
                        const size_t row = wr * 32 + a * 16 + l4 + 4 * q, col = wc * 32 + c * 16 + l15;
                        x[row][col] = G[(o + row) * ld + o + col] - accp[a][c][q];
                    }
        }
        gj_f64x4 accx[2][2];
        product(accx, oi, oj);     // X_b: G[bi, bj] - C[bi] R[:, bj]
        __syncthreads();
#pragma unroll
        for (int a = 0; a < 4; a++)
#pragma unroll
            for (int c = 0; c < 4; c++) r[a][c] = x[ty * 4 + a][tx * 4 + c];
        __syncthreads();
        const double keep = b == k - 1 ? 0. : 1.;   // the tile (k, k-1) lies in the pivot column of step k-1: -C P, no base
#pragma unroll
        for (int a = 0; a < 2; a++)
#pragma unroll
            for (int c = 0; c < 2; c++)
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const size_t row = wr * 32 + a * 16 + l4 + 4 * q, col = wc * 32 + c * 16 + l15;
                    // (keep = 0 instead of a select: a select lets the compiler branch around each load, and it then waited for the 16 loads one by one)
                    x[row][col] = G[(oi + row) * ld + oj + col] * keep - accx[a][c][q];
                }
    } else {
        for (int t = threadIdx.x; t < kGJ * kGJ; t += kBlock) {
            const int i = t / kGJ, j = t % kGJ;
            x[i][j] = G[(oi + i) * ld + oj + j];
        }
#pragma unroll
        for (int a = 0; a < 4; a++)
#pragma unroll
            for (int c = 0; c < 4; c++) r[a][c] = G[(o + ty * 4 + a) * ld + o + tx * 4 + c];
    }
    __syncthreads();
    for (int t = threadIdx.x; t < kGJ * kGJ; t += kBlock) {
        const int i = t / kGJ, j = t % kGJ;
        Cb[i * kGJ + j] = below ? x[i][j] : -x[j][i];
    }
    gj_invert64_scalar<4, SHM_GJ_STEP_PAIRS != 0>(r, scratch, flag);
#if SHM_GJ_STEP_MODE == 1
    if (b == k) {   // P_k = D_k^-1 goes to the block diagonal beside the factor
#pragma unroll
        for (int a = 0; a < 4; a++)
#pragma unroll
            for (int c = 0; c < 4; c++) Pd[(size_t)k * kGJ * kGJ + (ty * 4 + a) * kGJ + tx * 4 + c] = r[a][c];
        return;
    }
#endif
    if (b == k) {   // the pivot block's own R column carries P
#pragma unroll
        for (int a = 0; a < 4; a++)
#pragma unroll
            for (int c = 0; c < 4; c++) Rn[(size_t)(ty * 4 + a) * ld + ob + tx * 4 + c] = r[a][c];
        return;
    }
    // P: registers -> scratch, 8 rows at a time -> the lanes that feed it to the matrix cores (rows wr 32 + a 16 + l15, k = 4 s + l4)
    double pa[2][kGJ / 4];
#pragma unroll
    for (int pass = 0; pass < 8; pass++) {
        __syncthreads();
        if ((ty >> 1) == pass) {
#pragma unroll
            for (int a = 0; a < 4; a++)
#pragma unroll
                for (int c = 0; c < 4; c++) prow[(ty & 1) * 4 + a][tx * 4 + c] = r[a][c];
        }
        __syncthreads();
        if (wr == (pass >> 2) && (l15 >> 3) == (pass & 1)) {
#pragma unroll
            for (int s4 = 0; s4 < kGJ / 4; s4++) pa[(pass >> 1) & 1][s4] = prow[l15 & 7][4 * s4 + l4];
        }
    }
    gj_f64x4 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
        for (int c = 0; c < 2; c++) acc[a][c] = gj_f64x4{0., 0., 0., 0.};
#pragma unroll
    for (int s4 = 0; s4 < kGJ / 4; s4++) {
        const int kk = 4 * s4 + l4;
        double bf[2];
#pragma unroll
        for (int c = 0; c < 2; c++) {
            const int j = wc * 32 + c * 16 + l15;
            bf[c] = (b > k) ? x[j][kk] : x[kk][j];   // R[:, b] = P X^T below the pivot block, P X above it
        }
#pragma unroll
        for (int a = 0; a < 2; a++)
#pragma unroll
            for (int c = 0; c < 2; c++) acc[a][c] = __builtin_amdgcn_mfma_f64_16x16x4f64(pa[a][s4], bf[c], acc[a][c], 0, 0, 0);
    }
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
        for (int c = 0; c < 2; c++)
#pragma unroll
            for (int q = 0; q < 4; q++) Rn[(size_t)(wr * 32 + a * 16 + l4 + 4 * q) * ld + ob + wc * 32 + c * 16 + l15] = acc[a][c][q];
}
