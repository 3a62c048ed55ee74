// SNP association on the scan handle (gbrs_scan_set_snps / gbrs_scan_snp_dosage / gbrs_scan_snps; DESIGN.md §29): every
// founder SNP is tested with one degree of freedom on the allele dosage that its founder pattern implies.  Included by
// scan.hip inside namespace gbrs, after the product kernel's helpers.  There is no fused multiply-add anywhere (the
// library is built with -ffp-contract=off).
//
// Where a SNP lies.  A SNP has a chromosome c of the handle, a position x in the units of the grid positions and a
// founder pattern m (bit h set: founder h carries the alternative allele).  With g[0..k-1] the grid positions of the
// chromosome in the handle's point order (they must not decrease, and k >= 1):
//   lo = clip(searchsorted(g, x, 'right') - 1, 0, k-1),  hi = min(lo + 1, k-1)
//   t  = (x - g[lo]) / (g[hi] - g[lo]) if g[hi] > g[lo] and x > g[lo], else 0.0;  t = min(t, 1.0)
// so a SNP outside the grid takes the end point's dosage, as np.interp does, and a SNP on a duplicated grid position
// takes the last of the equal points.
// Its dosage for sample s.
//   a_lo = 0.0; for h ascending: if bit h of m: a_lo += D[s][lo][h];  a_hi likewise from D[s][hi]
//   x_s  = 2.0 * (a_lo + t * (a_hi - a_lo))
// The test, on a prepared handle (qz, c of gbrs_scan_prepare).  Every sum over the samples is one wavefront's, in
// scan_prepare_kernel's order: lane l adds the samples l, l + 64, ... in order and the 64 partial sums meet in the
// butterfly.
//   raw = sum x_s^2,  qtx[k] = sum_s qz[s][k] x_s
//   x~_s = x_s - sum_k (k ascending) qz[s][k] qtx[k],  G = sum x~_s^2
//   the SNP is used iff G > 0 and G > SC_PIVOT raw (§27's threshold with §27's meaning: a SNP that is monomorphic in the
//   cohort, the all-zeros and the all-ones pattern project to rounding and are not tested)
//   w = x~ / sqrt(G), a true division; zeros for an unused SNP
//   per phenotype p, y~ and rss0 as gbrs_scan_run forms them: ess = (w . y~_p)^2, lod = scan_lod(rss0, ess, n / 2)
//   an unused SNP has LOD 0.0 for every phenotype
//   peak_lod[p][c], peak_index[p][c]: the largest LOD over the used SNPs of chromosome c and that SNP's index in handle
//   order, the lowest on ties; NaN and -1 when the chromosome has no used SNP.

constexpr int SS_BLOCK = SC_ROWS;            // SNPs per workgroup of the row kernel: one row tile of the product
constexpr int64_t SS_CHUNK = 65536;          // SNPs whose rows w are on the device at a time
constexpr size_t SS_TABLE_BYTES = 20;        // per SNP on the handle: lo, hi (int32), pattern (uint32), t (double)
static_assert(SS_CHUNK % SC_ROWS == 0, "a chunk is whole row tiles, so a SNP's place in its tile does not depend on the chunk");

// One thread per SNP of the handle: its chromosome from the SNP offsets, then lo, hi as global point indices and t.
__global__ void __launch_bounds__(SC_THREADS)
scan_snp_locate_kernel(int64_t M_snp, int n_chrom, const int64_t *__restrict__ snp_off, const int64_t *__restrict__ point_off,
                       const double *__restrict__ g, const double *__restrict__ x, int32_t *__restrict__ lo,
                       int32_t *__restrict__ hi, double *__restrict__ t) {
    const int64_t j = (int64_t)blockIdx.x * SC_THREADS + threadIdx.x;
    if (j >= M_snp) return;
    int c = 0, c_end = n_chrom;
    while (c_end - c > 1) {
        const int mid = (c + c_end) / 2;
        if (snp_off[mid] <= j) c = mid;
        else c_end = mid;
    }
    const int64_t a = point_off[c], k = point_off[c + 1] - a;       // k >= 1: the host refused the others
    const double xx = x[j];
    int64_t below = 0, above = k;                                   // the number of g <= xx: searchsorted 'right'
    while (below < above) {
        const int64_t mid = (below + above) / 2;
        if (g[a + mid] <= xx) below = mid + 1;
        else above = mid;
    }
    const int64_t l = std::min(std::max<int64_t>(below - 1, 0), k - 1), h = std::min(l + 1, k - 1);
    const double gl = g[a + l], gh = g[a + h];
    double tt = (gh > gl && xx > gl) ? (xx - gl) / (gh - gl) : 0.0;
    tt = tt < 1.0 ? tt : 1.0;
    lo[j] = (int32_t)(a + l);
    hi[j] = (int32_t)(a + h);
    t[j] = tt;
}

// x_s of one SNP: the pattern's founders of the two points, `stride` doubles apart, in ascending order.
__device__ __forceinline__ double snp_dose(const double *__restrict__ lo, const double *__restrict__ hi, int64_t stride, int H,
                                           uint32_t mask, double t) {
    double a_lo = 0.0, a_hi = 0.0;
    for (int h = 0; h < H; ++h)
        if (mask >> h & 1u) {
            a_lo += lo[h * stride];
            a_hi += hi[h * stride];
        }
    return 2.0 * (a_lo + t * (a_hi - a_lo));
}

// out[s][j] = x_s of the SNPs first .. first + count - 1, one thread per value.
__global__ void __launch_bounds__(SC_THREADS)
scan_snp_dosage_kernel(int n, int64_t M, int H, int64_t first, int64_t count, const double *__restrict__ D,
                       const int32_t *__restrict__ lo, const int32_t *__restrict__ hi, const uint32_t *__restrict__ mask,
                       const double *__restrict__ t, double *__restrict__ out) {
    const int64_t idx = (int64_t)blockIdx.x * SC_THREADS + threadIdx.x;
    if (idx >= (int64_t)n * count) return;
    const int64_t s = idx / count, j = first + idx % count;
    out[idx] = snp_dose(D + (s * M + lo[j]) * H, D + (s * M + hi[j]) * H, 1, H, mask[j], t[j]);
}

// ---- the rows ------------------------------------------------------------------------------------------------------------------

// One workgroup per SS_BLOCK consecutive SNPs of the chunk, one wavefront per SNP at a time, so that every sum over the
// samples is one wavefront's.  The cohort is [n][M][H]: a point's rows are M H 8 bytes apart across the samples, so with
// `staged` the workgroup brings the two points of a run of SNPs that share (lo, hi) into LDS once, as pts[2][H][n]
// (the sample axis contiguous: lanes read consecutive words; rows n | 1 long), and its wavefronts take the run's SNPs in turn.  SNPs
// sorted by position come in such runs; a SNP whose neighbours lie elsewhere is a run of one.  Without `staged` (the
// two points do not fit the LDS) every SNP reads the cohort itself.  The arithmetic is the same either way.
//   1  x_s into the SNP's row of w, raw = sum x_s^2
//   2  qtx[k] = sum_s qz[s][k] x_s; lane k keeps qtx[k] (c <= 64)
//   3  x~_s = x_s - sum_k qz[s][k] qtx[k] in place, G = sum x~_s^2
//   4  used = G > 0 and G > SC_PIVOT raw;  w_s = x~_s / sqrt(G) or 0.0, zeros from sample n up to n_ld
// A lane writes and reads only its own samples of the row, so the steps need no barrier between them.  The loops over
// the samples run the whole wavefront through every lap (the tail is predicated), since step 3 reads other lanes.
__global__ void __launch_bounds__(SC_THREADS)
scan_snp_row_kernel(int n, int64_t M, int H, int c, int64_t n_ld, int64_t first, int64_t count, int staged,
                    const double *__restrict__ D, const double *__restrict__ qz, const int32_t *__restrict__ lo,
                    const int32_t *__restrict__ hi, const uint32_t *__restrict__ mask, const double *__restrict__ t,
                    double *__restrict__ w, uint8_t *__restrict__ used) {
    extern __shared__ double snp_pts[];        // [2][H][n_pad] with `staged`
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int n_pad = n | 1;                   // an odd row length: the staging's writes, n_pad words apart, spread over the banks
    const int64_t j0 = (int64_t)blockIdx.x * SS_BLOCK, j1 = std::min(j0 + SS_BLOCK, count);
    // the workgroup's SNPs are one wavefront wide: lane l of every wavefront holds the points of SNP j0 + l, and a run's end
    // comes from one ballot instead of a walk through memory
    static_assert(SS_BLOCK == 64, "one SNP of the workgroup per lane");
    const bool mine = j0 + lane < j1;
    const int32_t my_lo = mine ? lo[first + j0 + lane] : -1, my_hi = mine ? hi[first + j0 + lane] : -1;
    int64_t a = j0;
    while (a < j1) {                           // a run [a, b) of SNPs on one pair of points; a, b are the workgroup's
        const int at = (int)(a - j0);
        const int64_t plo = __shfl(my_lo, at, WAVE), phi = __shfl(my_hi, at, WAVE);
        const unsigned long long other = ~(__ballot(mine && my_lo == plo && my_hi == phi) >> at);      // bit 0 is clear: SNP a itself
        const int64_t b = a + (other ? __ffsll(other) - 1 : 64 - at);
        if (staged) {
            __syncthreads();                   // the last run's readers are done
            // sixteen lanes across a sample's H <= 17 founders (contiguous in the cohort), sixteen samples per lap
            const int h = tid & 15;
            for (int s = tid >> 4; s < n; s += SC_THREADS / 16)
                for (int hh = h; hh < H; hh += 16) {
                    snp_pts[(int64_t)hh * n_pad + s] = D[((int64_t)s * M + plo) * H + hh];
                    snp_pts[(int64_t)(H + hh) * n_pad + s] = D[((int64_t)s * M + phi) * H + hh];
                }
            __syncthreads();
        }
        for (int64_t j = a + wave; j < b; j += SC_THREADS / 64) {
            const uint32_t m = mask[first + j];
            const double tt = t[first + j];
            double *wr = w + j * n_ld;
            double raw = 0.0;
            for (int s = lane; s < n; s += 64) {
                const double x = staged ? snp_dose(snp_pts + s, snp_pts + (int64_t)H * n_pad + s, n_pad, H, m, tt)
                                        : snp_dose(D + ((int64_t)s * M + plo) * H, D + ((int64_t)s * M + phi) * H, 1, H, m, tt);
                wr[s] = x;
                raw += x * x;
            }
            raw = wave_sum_all(raw);
            double q_mine = 0.0;               // qtx[lane]
            for (int k = 0; k < c; ++k) {
                double acc = 0.0;
                for (int s = lane; s < n; s += 64) acc += qz[(int64_t)s * c + k] * wr[s];
                acc = wave_sum_all(acc);
                if (lane == k) q_mine = acc;
            }
            double G = 0.0;
            for (int s0 = 0; s0 < n; s0 += 64) {
                const int s = s0 + lane;
                const bool in = s < n;
                double p = 0.0;
                for (int k = 0; k < c; ++k) {
                    const double q = __shfl(q_mine, k, WAVE);
                    p += (in ? qz[(int64_t)s * c + k] : 0.0) * q;
                }
                if (in) {
                    const double v = wr[s] - p;
                    wr[s] = v;
                    G += v * v;
                }
            }
            G = wave_sum_all(G);
            const bool ok = G > 0.0 && G > SC_PIVOT * raw;
            const double r = sqrt(G);
            for (int64_t s = lane; s < n_ld; s += 64) wr[s] = (ok && s < n) ? wr[s] / r : 0.0;
            if (lane == 0) used[j] = ok ? 1 : 0;
        }
        a = b;
    }
}

// ---- the product ---------------------------------------------------------------------------------------------------------------

// scan_lod_kernel with one row per SNP: the same operand maps, LDS stride, K chunks and prefetch; blockIdx.x: block of 64
// SNP rows of the chunk, blockIdx.y: block of 64 phenotypes.  Every MFMA row is a SNP.  The epilogue squares the
// accumulator - ess of (row, column) is one register of one lane, no cross-lane sum - and passes it through LDS as
// [column][row] (stride 65: the sixteen lanes of a group write sixteen columns); every thread then turns sixteen of the
// 64 x 64 values into LODs, consecutive threads consecutive SNPs of one phenotype's row.  Rows past the chunk and columns
// past P shadow the last valid one and are not stored.  lod is the chunk's [P][ld].
__global__ void __launch_bounds__(SC_THREADS)
scan_snp_lod_kernel(int64_t rows, int64_t P, int64_t n_ld, int64_t ld, double half_n, const double *__restrict__ w,
                    const double *__restrict__ yt, const double *__restrict__ rss0, double *__restrict__ lod) {
    constexpr int ESS_LD = SC_ROWS + 1;
    __shared__ __attribute__((aligned(16))) double lds[(SC_ROWS + SC_COLS) * SC_LD];
    static_assert(SC_COLS * ESS_LD <= (SC_ROWS + SC_COLS) * SC_LD, "the epilogue's [column][row] fits the operands' LDS");
    double *lds_a = lds, *lds_b = lds + SC_ROWS * SC_LD;
    const int64_t row0 = (int64_t)blockIdx.x * SC_ROWS, col0 = (int64_t)blockIdx.y * SC_COLS;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, i = lane & 15, g = lane >> 4;
    scan_d4 acc[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) acc[u] = scan_d4{0.0, 0.0, 0.0, 0.0};
    const double *ra = lds_a + (wave * 16 + i) * SC_LD + g, *rb = lds_b + i * SC_LD + g;
    auto multiply = [&]() {
#pragma unroll
        for (int kk = 0; kk < SC_KC; kk += 4) {
            const double av = ra[kk];
#pragma unroll
            for (int u = 0; u < 4; ++u) acc[u] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, rb[u * 16 * SC_LD + kk], acc[u], 0, 0, 0);
        }
    };
    const int64_t chunks = n_ld / SC_KC;       // >= 1
    double va[SC_PER], vb[SC_PER];
    scan_fetch(va, w, n_ld, row0, rows);
    scan_fetch(vb, yt, n_ld, col0, P);
    for (int64_t k = 1; k < chunks; ++k) {
        scan_put(lds_a, va);
        scan_put(lds_b, vb);
        __syncthreads();
        scan_fetch(va, w + k * SC_KC, n_ld, row0, rows);
        scan_fetch(vb, yt + k * SC_KC, n_ld, col0, P);
        multiply();
        __syncthreads();
    }
    scan_put(lds_a, va);
    scan_put(lds_b, vb);
    __syncthreads();
    multiply();
    __syncthreads();
    double *ess = lds;                         // [64 columns][ESS_LD]
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int r = 0; r < 4; ++r) ess[(u * 16 + i) * ESS_LD + wave * 16 + g + 4 * r] = acc[u][r] * acc[u][r];
    __syncthreads();
#pragma unroll
    for (int u = 0; u < SC_COLS * SC_ROWS / SC_THREADS; ++u) {
        const int idx = threadIdx.x + SC_THREADS * u, col = idx / SC_ROWS, row = idx % SC_ROWS;
        const int64_t j = row0 + row, p = col0 + col;
        if (j < rows && p < P) lod[p * ld + j] = scan_lod(rss0[p], ess[col * ESS_LD + row], half_n);
    }
}

// ---- peaks -----------------------------------------------------------------------------------------------------------------------

// One wavefront per (chromosome, phenotype of the phenotype chunk), once per SNP chunk [first, first + count): lane l looks
// at the used SNPs l, l + 64, ... of the chromosome's share of the chunk and keeps the first of its largest; the 64
// candidates meet in scan_peak_kernel's butterfly (the larger value, the lower index).  The winner replaces what the
// chunks before left in peak_lod / peak_index only when it is larger: the chunks come in ascending order, so the carried
// index is the lower one.  peak_index starts at -1; no atomics.
__global__ void __launch_bounds__(64)
scan_snp_peak_kernel(int64_t first, int64_t count, int64_t ld, int n_chrom, const int64_t *__restrict__ snp_off,
                     const uint8_t *__restrict__ used, const double *__restrict__ lod, double *__restrict__ peak_lod,
                     int64_t *__restrict__ peak_index) {
    const int c = blockIdx.x;
    const int64_t p = blockIdx.y, lo = std::max(snp_off[c], first), hi = std::min(snp_off[c + 1], first + count);
    double best = -__builtin_huge_val();
    int64_t at = -1;
    for (int64_t j = lo + threadIdx.x; j < hi; j += 64) {
        if (!used[j - first]) continue;
        const double v = lod[p * ld + (j - first)];
        if (at < 0 || v > best) {
            best = v;
            at = j;
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double ov = __shfl_xor(best, off, WAVE);
        const int64_t oa = __shfl_xor((long long)at, off, WAVE);
        if (oa >= 0 && (at < 0 || ov > best || (ov == best && oa < at))) {
            best = ov;
            at = oa;
        }
    }
    if (threadIdx.x == 0 && at >= 0) {
        const int64_t slot = p * n_chrom + c;
        if (peak_index[slot] < 0 || best > peak_lod[slot]) {
            peak_lod[slot] = best;
            peak_index[slot] = at;
        }
    }
}
