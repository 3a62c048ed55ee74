// Multiread models 1-3 (emase/EMfactory.py:160-203), included from em.hip inside namespace gbrs.
//
// Every division of those models is elementwise on the stored entries of the numerator, so an E-step never needs the
// per-entry posterior either: for a stored entry (read r, haplotype h, locus l of gene g) the posterior is
// theta[h,l] * f / D_r with
//       model 3   f = T_g / S[r,g]
//       model 2   f = U_l T_g / (V[r,l] W[r,g])
//       model 1   f = Y[h,g] T_g / (X[r,g,h] Z[r,g])
//   T_g = sum of theta over gene g, Y[h,g] = the same for haplotype h, U_l = sum of theta over the haplotypes of l,
//   S[r,g] = sum of theta over the read's entries in g, V[r,l] over its entries of locus l, X[r,g,h] over its entries
//   of haplotype h in g, W[r,g] = sum of U over the loci it touches in g, Z[r,g] = sum of Y[., g] over the haplotypes
//   it touches in g, and D_r = sum of T_g over the genes it touches.
// An entry whose theta is 0 takes no part in any of these sums (the reference eliminates zeros before each
// division).  A[h,l] = sum over the reads of count[r] f / D_r then goes through the Model-4 M-step unchanged.
//
// The grouped row layout (em_layout.hip build_grouped_order) holds every stored entry sorted by (row, gene, locus,
// haplotype) for models 2 and 3, by (row, gene, haplotype, locus) for model 1, so that every (read, gene) segment and
// inside it every (locus) or (haplotype) run is contiguous.  Per step:
//   model_totals_kernel   T, Y (gene-major, g * H + h) and U from the locus-major theta
//   model_row_kernel      one lane per read walks its segments and stores each entry's count * f / D at the entry's
//                         CSC position
//   model_col_kernel      the CSC entries in order: a column's factors are summed across the wavefront before one
//                         atomic per column chunk (as csc_acc_kernel)
// The factors stay in `fac` until the next step of one of these models (a step the stopping rule turned into a no-op
// leaves them alone): gbrs_em_posterior (em.hip, post_value_kernel) reads them back, divides the count out again and
// multiplies by the theta the step started from.

__global__ void __launch_bounds__(256)
model_totals_kernel(uint32_t L, uint32_t H, uint32_t n_genes, const uint32_t *__restrict__ gene_ptr,
                    const uint32_t *__restrict__ gene_mem, const double *__restrict__ theta, double *__restrict__ T,
                    double *__restrict__ Y, double *__restrict__ U, const EmScalars *__restrict__ sc) {
    if (sc->stop) return;
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < L) {
        double u = 0.0;
        for (uint32_t h = 0; h < H; ++h) u += theta[(size_t)i * H + h];
        U[i] = u;
    }
    if (i < n_genes) {
        const uint32_t a = gene_ptr[i], b = gene_ptr[i + 1];
        double t = 0.0;
        for (uint32_t h = 0; h < H; ++h) {
            double y = 0.0;
            for (uint32_t m = a; m < b; ++m) y += theta[(size_t)gene_mem[m] * H + h];
            Y[(size_t)i * H + h] = y;
            t += y;
        }
        T[i] = t;
    }
}

template <int MODEL>
__device__ __forceinline__ uint32_t model_run_key(uint32_t w) {
    return MODEL == 2 ? (w >> 5) : MODEL == 1 ? (w & 31u) : 0u;      // runs: one locus / one haplotype / the segment
}

template <int MODEL>
__global__ void __launch_bounds__(256)
model_row_kernel(uint64_t R, uint32_t H, const uint32_t *__restrict__ row_ptr, const uint32_t *__restrict__ lh,
                 const uint32_t *__restrict__ src, const uint32_t *__restrict__ locus_gene,
                 const double *__restrict__ theta, const double *__restrict__ T, const double *__restrict__ Y,
                 const double *__restrict__ U, const double *__restrict__ count, double *__restrict__ fac,
                 const EmScalars *__restrict__ sc) {
    if (sc->stop) return;
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= R) return;
    const uint32_t a = row_ptr[r], b = row_ptr[r + 1];
    if (a == b) return;
    auto th = [&](uint32_t w) { return theta[(size_t)(w >> 5) * H + (w & 31u)]; };
    // D_r: the totals of the genes the read touches with a nonzero theta
    double D = 0.0;
    uint32_t g_prev = locus_gene[lh[a] >> 5];
    bool touched = false;
    for (uint32_t j = a; j < b; ++j) {
        const uint32_t w = lh[j], g = locus_gene[w >> 5];
        if (g != g_prev) {
            if (touched) D += T[g_prev];
            g_prev = g;
            touched = false;
        }
        touched |= th(w) > 0.0;
    }
    if (touched) D += T[g_prev];
    const double cnt = count ? count[r] : 1.0;
    for (uint32_t s = a; s < b;) {
        const uint32_t g = locus_gene[lh[s] >> 5];
        uint32_t e = s + 1;
        while (e < b && locus_gene[lh[e] >> 5] == g) ++e;
        // S (model 3), W (model 2) or Z (model 1) of the segment [s, e)
        double outer = 0.0;
        for (uint32_t p = s; p < e;) {
            const uint32_t key = model_run_key<MODEL>(lh[p]);
            double sum = 0.0;
            uint32_t q = p;
            for (; q < e && model_run_key<MODEL>(lh[q]) == key; ++q) sum += th(lh[q]);
            if (MODEL == 3) outer += sum;
            else if (sum > 0.0) outer += MODEL == 2 ? U[lh[p] >> 5] : Y[(size_t)g * H + (lh[p] & 31u)];
            p = q;
        }
        const double Tg = T[g];
        for (uint32_t p = s; p < e;) {
            const uint32_t key = model_run_key<MODEL>(lh[p]);
            uint32_t q = p;
            double run = 0.0;                    // V (model 2), X (model 1)
            for (; q < e && model_run_key<MODEL>(lh[q]) == key; ++q) run += th(lh[q]);
            double f;
            if (MODEL == 3) f = Tg / outer;
            else if (MODEL == 2) f = U[lh[p] >> 5] * Tg / (run * outer);
            else f = Y[(size_t)g * H + (lh[p] & 31u)] * Tg / (run * outer);
            const double v = cnt * f / D;
            for (uint32_t j = p; j < q; ++j) fac[src[j]] = th(lh[j]) > 0.0 ? v : 0.0;
            p = q;
        }
        s = e;
    }
}

__global__ void __launch_bounds__(256)
model_col_kernel(uint64_t n, uint32_t ncols, uint32_t L, uint32_t H, const uint64_t *__restrict__ col_ptr,
                 const double *__restrict__ fac, double *__restrict__ acc, const EmScalars *__restrict__ sc) {
    if (sc->stop) return;
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k - (threadIdx.x & 63) >= n) return;
    const bool live = k < n;
    const uint32_t c = entry_column(col_ptr, ncols, live ? k : n - 1, n);
    const double w = live ? fac[k] : 0.0;
    const uint32_t c0 = __shfl(c, 0, WAVE);
    if (__all(c == c0)) {
        const double s = wave_sum(w);
        if ((threadIdx.x & 63) == 0) {
            const uint32_t h = c0 / L, l = c0 - h * L;
            atomicAdd(&acc[(size_t)l * H + h], s);
        }
    } else if (live) {
        const uint32_t h = c / L, l = c - h * L;
        atomicAdd(&acc[(size_t)l * H + h], w);
    }
}
