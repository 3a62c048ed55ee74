// SNP imputation of the HMM handle (gbrs_hmm_set_snps / gbrs_hmm_impute; DESIGN.md §26): the expected number of
// alternative alleles of every sample at every SNP, from the posteriors that gbrs_hmm_run left in HBM and the SNP's
// founder allele pattern.  The SNPs of a chromosome are a grid (grid_knots.h); the pattern folds the founder axis away
// before the interpolation, so no H-wide or S-wide value of a SNP reaches HBM.  Included by hmm_passes.hip inside namespace gbrs.

constexpr int IMPUTE_THREADS = 256;

// Once per gbrs_hmm_set_snps, one lane per SNP: grid_kernel's binary search, stored as the index of the knot above the SNP
// in the handle's knot arrays (knot_off + searchsorted(knots, x, 'left') clipped to [1, n_knots - 1]).  knot_row, made
// on the host beside the knots, is the gene row (gene_off + knot_gene) of every knot, so the imputation kernel needs
// neither the chromosome table nor a search.
__global__ void __launch_bounds__(IMPUTE_THREADS)
snp_setup_kernel(int n_chrom, int64_t n_snps, const SnpChrom *__restrict__ chroms, const double *__restrict__ knots,
                 const double *__restrict__ snp_x, int32_t *__restrict__ snp_idx) {
    const int64_t k = (int64_t)blockIdx.x * IMPUTE_THREADS + threadIdx.x;
    if (k >= n_snps) return;
    int c = 0;                                     // the last chromosome with SNPs whose first SNP is at or before k
    for (int j = 0; j < n_chrom; ++j)
        if (chroms[j].n_knots > 0 && chroms[j].snp_off <= k) c = j;
    const SnpChrom ch = chroms[c];
    const double *xs = knots + ch.knot_off;
    const double x = snp_x[k];
    int lo = 0, hi = ch.n_knots;                   // searchsorted(xs, x, side='left')
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (xs[mid] < x) lo = mid + 1; else hi = mid;
    }
    snp_idx[k] = ch.knot_off + min(max(lo, 1), ch.n_knots - 1);
}

// sum over the founders h of the pattern, ascending, of a row of D.  `acc += bit ? d : 0.0` gives the bits of the
// branching loop: the terms are >= 0 and acc starts at +0.0.  VEC2: rows are 16-byte aligned (even H).  HC: the founder
// count when the kernel is compiled for one (8: the loop unrolls and the lane masks of the pattern's bits are made once,
// outside the sample loop), 0: H is read at run time.
template <bool VEC2, int HC>
__device__ __forceinline__ double impute_fold(const double *__restrict__ row, int H, uint32_t m) {
    const int Hn = HC ? HC : H;
    double acc = 0.0;
    if (VEC2) {
        const double2 *r2 = reinterpret_cast<const double2 *>(row);
#pragma unroll
        for (int h = 0; h < Hn; h += 2) {
            const double2 d = r2[h >> 1];
            acc += (m >> h) & 1u ? d.x : 0.0;
            acc += (m >> (h + 1)) & 1u ? d.y : 0.0;
        }
    } else {
        for (int h = 0; h < Hn; ++h) acc += (m >> h) & 1u ? row[h] : 0.0;
    }
    return acc;
}

constexpr int IMPUTE_SAMPLES = 8;    // samples per workgroup: launches of few SNPs still fill the chip

// The samples s0 .. s1 of one lane's SNP: two rows of D, folded, interpolated (interpolate_kernel's order), doubled, stored.
template <bool VEC2, int HC>
__device__ __forceinline__ void impute_samples(const double *__restrict__ r_lo, const double *__restrict__ r_hi, int H, uint32_t m,
                                               double dx, double w, int64_t sample_stride, int s0, int s1,
                                               double *__restrict__ out, int64_t count) {
    for (int s = s0; s < s1; ++s) {
        const double a_lo = impute_fold<VEC2, HC>(r_lo, H, m), a_hi = impute_fold<VEC2, HC>(r_hi, H, m);
        const double slope = (a_hi - a_lo) / w;
        const double y = slope * dx + a_lo;
        out[(int64_t)s * count] = 2.0 * y;
        r_lo += sample_stride;
        r_hi += sample_stride;
    }
}

// Lanes across the SNPs first .. first + count, blockIdx.y across groups of IMPUTE_SAMPLES samples.  A lane loads what
// does not depend on the sample once - its position, pattern, the two knots around it and their gene rows - then walks
// its samples: two rows of H consecutive doubles of D[n][total_genes][H], folded with the pattern, interpolated
// (slope = (a_hi - a_lo) / (x_hi - x_lo); y = slope * (x - x_lo) + a_lo), doubled, and one store to out[s][snp],
// coalesced across the lanes.  Where SNPs outnumber genes most wavefronts lie between one pair of knots: such a
// wavefront reads its two rows through addresses that are the same in every lane, once for all 64 lanes, instead of
// 64 times through the vector memory path, which is what bounds the other branch.  Both branches take the same
// operations on the same numbers.
template <bool VEC2, int HC>
__global__ void __launch_bounds__(IMPUTE_THREADS)
impute_kernel(int H, int n, int64_t total_genes, int64_t first, int64_t count, const double *__restrict__ knots,
              const int32_t *__restrict__ knot_row, const double *__restrict__ snp_x, const uint32_t *__restrict__ snp_mask,
              const int32_t *__restrict__ snp_idx, const double *__restrict__ D, double *__restrict__ out) {
    const int64_t k = (int64_t)blockIdx.x * IMPUTE_THREADS + threadIdx.x;
    if (k >= count) return;
    const int s0 = (int)blockIdx.y * IMPUTE_SAMPLES, s1 = min(n, s0 + IMPUTE_SAMPLES);
    const int32_t idx = snp_idx[first + k];
    const double x = snp_x[first + k];
    const uint32_t m = snp_mask[first + k];
    const double x_lo = knots[idx - 1], x_hi = knots[idx];
    const double dx = x - x_lo, w = x_hi - x_lo;
    const int64_t sample_stride = total_genes * H;
    const double *base = D + (int64_t)s0 * sample_stride;
    const int32_t idx0 = __builtin_amdgcn_readfirstlane(idx);
    if (__all(idx == idx0)) {
        const double *r_lo = base + (int64_t)knot_row[idx0 - 1] * H, *r_hi = base + (int64_t)knot_row[idx0] * H;
        impute_samples<VEC2, HC>(r_lo, r_hi, H, m, dx, w, sample_stride, s0, s1, out + k, count);
    } else {
        const double *r_lo = base + (int64_t)knot_row[idx - 1] * H, *r_hi = base + (int64_t)knot_row[idx] * H;
        impute_samples<VEC2, HC>(r_lo, r_hi, H, m, dx, w, sample_stride, s0, s1, out + k, count);
    }
}
