// Grid pass of the HMM handle (gbrs_hmm_set_grid / gbrs_hmm_grid; DESIGN.md §21): the posteriors that gbrs_hmm_run left
// in HBM, interpolated onto the marker grid (`gbrs interpolate`, gbrs_utils.py:664-688) and reduced to founder dosages
// (`gbrs export`, :888-927) for every (sample, chromosome) of the run in one launch.  Included by hmm_passes.hip inside
// namespace gbrs.

// Grid points per tile: 64 where a tile of 64 rows of S | 1 doubles stays under 32 KB of LDS (S <= 63), else 32
// (S = 136: 35 KB, four workgroups per CU).
inline int grid_tile_points(int S) { return S <= 63 ? 64 : 32; }
inline size_t grid_tile_lds(int S) {
    const int P = grid_tile_points(S);
    return (size_t)P * (S | 1) * sizeof(double) + (size_t)P * sizeof(int32_t);
}

// One wavefront per (tile, sample).  Consecutive grid points mostly fall between the same two genes (64k points over 40k
// genes), so the wave walks its points in order with lanes across the states: the two gene rows of a segment are read
// coalesced (S contiguous doubles each) when the segment changes and stay in registers while it lasts; a step to the next
// segment keeps the upper row as the new lower one.  The interpolated states of the tile go to LDS, rows S | 1 doubles
// apart: lanes across states write consecutive banks, and the readers below, lanes across grid points, are an odd
// stride apart, so neither side conflicts.  From LDS they are
//   - reduced to H dosages per grid point, every sum by one lane over the states in state order, which is dosage_kernel's
//     loop, and stored as P * H consecutive doubles;
//   - and / or written out transposed as (S x n_points) rows, lanes across grid points.
// With the dosage alone no S-wide value of a grid point reaches HBM.
// Operation order (the library is built with -ffp-contract=off):  searchsorted(knots, x, side='left') clipped to
// [1, n_knots - 1];  slope = (y_hi - y_lo) / (x_hi - x_lo);  y = slope * (x - x_lo) + y_lo  (interpolate_kernel's);
// acc += p[g] * (0.5 * ((a == h) + (b == h))) over g = (a, b) in state order (dosage_kernel's).
// NCH = ceil(S / 64) states per lane.
template <int NCH>
__global__ void __launch_bounds__(64)
grid_kernel(int H, int S, int P, int64_t total_genes, int64_t total_points, int sample0,
            const GridChrom *__restrict__ chroms, const GridTile *__restrict__ tiles, const double *__restrict__ knots,
            const int32_t *__restrict__ knot_gene, const double *__restrict__ points, const double *__restrict__ gamma,
            double *__restrict__ dosage, double *__restrict__ gamma_grid) {
    extern __shared__ double grid_lds[];
    const int lane = threadIdx.x;
    const GridTile t = tiles[blockIdx.x];
    const GridChrom c = chroms[t.chrom];
    const int LD = S | 1;
    double *tile = grid_lds;                                            // [P][LD]
    int32_t *seg = reinterpret_cast<int32_t *>(grid_lds + (size_t)P * LD);   // [P]: the knot above each grid point
    const int np = min(P, c.n_points - t.first);
    const double *xs = knots + c.knot_off;
    const int32_t *kg = knot_gene + c.knot_off;
    const double *xq = points + c.point_off + t.first;
    if (lane < np) {
        const double x = xq[lane];
        int lo = 0, hi = c.n_knots;                // searchsorted(xs, x, side='left')
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (xs[mid] < x) lo = mid + 1; else hi = mid;
        }
        seg[lane] = min(max(lo, 1), c.n_knots - 1);
    }
    __syncthreads();
    const double *rows = gamma + ((int64_t)(sample0 + (int)blockIdx.y) * total_genes + c.gene_off) * S;
    double y_lo[NCH], y_hi[NCH];
    int cur = -1;
    for (int p = 0; p < np; ++p) {
        const int idx = __builtin_amdgcn_readfirstlane(seg[p]);
        if (idx != cur) {
            const bool next = idx == cur + 1;
            const double *r_lo = rows + (int64_t)kg[idx - 1] * S, *r_hi = rows + (int64_t)kg[idx] * S;
#pragma unroll
            for (int k = 0; k < NCH; ++k) {
                const int s = lane + 64 * k;
                if (s < S) {
                    y_lo[k] = next ? y_hi[k] : r_lo[s];
                    y_hi[k] = r_hi[s];
                }
            }
            cur = idx;
        }
        const double x = xq[p], x_lo = xs[idx - 1], x_hi = xs[idx];
#pragma unroll
        for (int k = 0; k < NCH; ++k) {
            const int s = lane + 64 * k;
            if (s < S) {
                const double slope = (y_hi[k] - y_lo[k]) / (x_hi - x_lo);
                tile[p * LD + s] = slope * (x - x_lo) + y_lo[k];
            }
        }
    }
    __syncthreads();
    const int64_t out_sample = blockIdx.y;
    if (dosage) {
        double *out = dosage + (out_sample * total_points + c.point_off + t.first) * H;
        for (int q = lane; q < np * H; q += 64) {
            const int p = q / H, h = q - p * H;
            const double *pr = tile + p * LD;
            double acc = 0.0;
            int g = 0;
            for (int a = 0; a < H; ++a)
                for (int b = a; b < H; ++b, ++g) {
                    const double w = 0.5 * ((a == h) + (b == h));
                    acc += pr[g] * w;
                }
            out[q] = acc;
        }
    }
    if (gamma_grid) {
        // the (S x n_points) block of this (sample, chromosome): the samples S * total_points apart, the chromosomes of a
        // sample one after the other
        double *out = gamma_grid + (out_sample * total_points + c.point_off) * S + t.first;
        const int p = lane & (P - 1), s0 = lane / P, step = 64 / P;
        if (p < np)
            for (int s = s0; s < S; s += step) out[(int64_t)s * c.n_points + p] = tile[p * LD + s];
    }
}
