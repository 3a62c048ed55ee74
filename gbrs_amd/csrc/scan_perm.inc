// Permutation thresholds of the genome scan (gbrs_scan_permute; DESIGN.md §28).  Included by scan.hip inside namespace
// gbrs, after the kernels of the plain scan: the permuted columns go through scan_lod_kernel and scan_peak_kernel as
// any phenotype column does.

constexpr int SP_THREADS = 256;

// The key of sample s in permutation b: words 0 and 1 of Philox4x32-10 on the counter (s, b) under the seed.
__device__ __forceinline__ uint64_t scan_perm_key(uint64_t s, uint64_t b, uint32_t k0, uint32_t k1) {
    uint32_t c[4] = {(uint32_t)s, (uint32_t)(s >> 32), (uint32_t)b, (uint32_t)(b >> 32)};
    philox4x32_10(c, k0, k1);
    return ((uint64_t)c[0] << 32) | c[1];
}

// perm[b][s] = the rank of (key_s, s) among the n pairs of permutation b, by counting: workgroup (tile, b) holds 256
// samples, one per thread, and walks all n keys in tiles of 256 through LDS; a thread counts the pairs below its own.
// The keys are recomputed per tile instead of being kept: n / 256 Philox calls per sample next to n comparisons.  n^2
// comparisons per permutation: 0.26 M at 512 samples.  blockIdx.x = b * tiles + tile.
__global__ void __launch_bounds__(SP_THREADS)
scan_perm_rank_kernel(int n, int tiles, uint32_t k0, uint32_t k1, int32_t *__restrict__ perm) {
    __shared__ uint64_t keys[SP_THREADS];
    const int64_t b = blockIdx.x / tiles;
    const int s = (int)(blockIdx.x % tiles) * SP_THREADS + threadIdx.x;      // < n + 256 <= 2^27 + 256
    const uint64_t mine = scan_perm_key((uint64_t)s, (uint64_t)b, k0, k1);
    int below = 0;
    for (int t0 = 0; t0 < n; t0 += SP_THREADS) {
        __syncthreads();
        keys[threadIdx.x] = scan_perm_key((uint64_t)(t0 + threadIdx.x), (uint64_t)b, k0, k1);   // past n: not compared
        __syncthreads();
        const int m = min(SP_THREADS, n - t0);
        for (int j = 0; j < m; ++j) {
            const uint64_t k = keys[j];
            below += (k < mine || (k == mine && t0 + j < s)) ? 1 : 0;
        }
    }
    if (s < n) perm[b * n + s] = below;
}

// The sibling of scan_pheno_kernel for column col0 + blockIdx.x = p B + b of the pass: y*[s] = y~_p[perm_b[s]] read from the
// resident projected phenotypes yt_all [P][n_ld], then y*~ = y* - qz qz' y* into row blockIdx.x of yt and rss0 = |y*~|^2,
// every sum in scan_pheno_kernel's order (lane l adds the samples l, l + 64, ..., the partial sums meet in a butterfly).
__global__ void __launch_bounds__(64)
scan_perm_pheno_kernel(int n, int c, int64_t n_ld, int64_t B, int64_t col0, const double *__restrict__ yt_all,
                       const int32_t *__restrict__ perm, const double *__restrict__ qz, double *__restrict__ yt,
                       double *__restrict__ rss0) {
    __shared__ double qty[SC_MAX_C];
    const int64_t col = col0 + blockIdx.x, p = col / B, b = col % B, row = blockIdx.x;
    const double *src = yt_all + p * n_ld;
    const int32_t *pi = perm + b * n;
    const int lane = threadIdx.x;
    for (int k = 0; k < c; ++k) {
        double acc = 0.0;
        for (int s = lane; s < n; s += 64) acc += qz[(int64_t)s * c + k] * src[pi[s]];
        acc = wave_sum_all(acc);
        if (lane == 0) qty[k] = acc;
    }
    __syncthreads();
    double ss = 0.0;
    for (int64_t s = lane; s < n_ld; s += 64) {
        double v = 0.0;
        if (s < n) {
            double proj = 0.0;
            for (int k = 0; k < c; ++k) proj += qz[s * c + k] * qty[k];
            v = src[pi[s]] - proj;
        }
        yt[row * n_ld + s] = v;
        ss += v * v;
    }
    ss = wave_sum_all(ss);
    if (lane == 0) rss0[row] = ss;
}

// perm_max of the chunk's columns: one thread per column takes the largest of its per-chromosome peaks over the selected
// chromosomes that hold points (an empty one's peak is NaN and is not looked at).  No atomics.
__global__ void __launch_bounds__(SP_THREADS)
scan_perm_max_kernel(int64_t cols, int n_chrom, const int64_t *__restrict__ point_off, const uint8_t *__restrict__ mask,
                     const double *__restrict__ peak_lod, double *__restrict__ out) {
    const int64_t col = (int64_t)blockIdx.x * SP_THREADS + threadIdx.x;
    if (col >= cols) return;
    double best = -__builtin_huge_val();
    for (int c = 0; c < n_chrom; ++c)
        if (mask[c] && point_off[c + 1] > point_off[c]) {
            const double v = peak_lod[col * n_chrom + c];
            if (v > best) best = v;
        }
    out[col] = best;
}
