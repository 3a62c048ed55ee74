// SNP association under the mixed model on the scan handle (gbrs_scan_lmm_snps; DESIGN.md §33; R/qtl2's
// scan1snps(..., kinship = loco)): §29's one-degree-of-freedom test of every founder SNP with §32's polygenic effect.
// Included by scan.hip inside namespace gbrs, after scan_snp.inc and scan_lmm.inc.  There is no fused multiply-add anywhere
// (the library is built with -ffp-contract=off).
//
// The rule, on a handle that holds SNPs (gbrs_scan_set_snps) and a mixed-model preparation (gbrs_scan_lmm_prepare):
//   1  dosage    x_s of SNP j is §29's: snp_dose, the function gbrs_scan_snp_dosage uses, so the bits are the same
//   2  rotation  e = eig_of_chrom[chromosome of j], x* = U_e' x: one accumulator chain per entry over the samples in the
//                order of the K chunks, as lmm_rotate_kernel forms R_m
//   3  null fit  per (phenotype p, decomposition e) gbrs_scan_lmm_run's, by its kernel, hsq_in honoured, the phenotype
//                column centred by the caller: sw = v^-1/2, Qz (cz columns), y~ and rss0
//   4  columns   g = sw . y~,  o = sw . sw,  c_k = sw . Qz_k
//   5  sums per (j, p), each one chain over the samples in ascending K-chunk order that depends on the SNP's row and the
//      phenotype's column alone:
//                b = sum_i x*_i g_i,  raw = sum_i (x*_i x*_i) o_i,  qtx_k = sum_i x*_i c_k,i
//   6  the test  S = 0.0; for k ascending: S += qtx_k * qtx_k;  G = raw - S
//                the pair is used iff G > 0 and G > SC_PIVOT raw (§29's meaning)
//                ess = b * b / G, a true division;  lod = scan_lod(rss0, ess, n / 2) with both edge rules
//                a pair that is not used gives exactly 0.0; the column of zeros (rss0 = 0) gives 0.0 everywhere
//   7  peaks     peak_lod[p][c], peak_index[p][c]: the largest LOD over the used SNPs of chromosome c, the lowest index
//                on ties; NaN and -1 when there is none.  n_used[p][c] counts the used ones.
// `used` depends on the phenotype, because the weights do: it is [P][M_snp].  G is a difference of sums; that is the
// rule, not an accident: |x~|^2 = |x^|^2 - |Qz' x^|^2 for an orthonormal Qz, and the two sums are linear and quadratic in
// x*, so the whole test is a few f64 MFMA products of the SNP rows with columns the null fit already made.

constexpr int LS_GROUP = 2;                  // covariate columns a K sweep accumulates beside each other
constexpr int LS_MAX_B = LS_GROUP + 2;       // B operand blocks of the first sweep: g, o and the first group
constexpr size_t LS_LDS_BYTES = (size_t)(SC_ROWS + LS_MAX_B * SC_COLS) * SC_LD * sizeof(double);
constexpr int LS_OUT_LD = SC_ROWS + 1;       // the epilogue's [column][row] stride, scan_snp_lod_kernel's
static_assert((size_t)SC_COLS * LS_OUT_LD * (sizeof(double) + 1) <= LS_LDS_BYTES, "the epilogue's LODs and flags fit the operands' LDS");

// ---- columns -------------------------------------------------------------------------------------------------------------------

// One thread per (phenotype of the chunk, decomposition, rotated sample): the null fit's sw, qz and yt ([pc n_eig] rows,
// lmm_null_kernel's order) become the product's B operands, kept for all P as cols[e][q][P][n_ld] with q = 0: g, 1: o,
// 2 + k: c_k.  The padding past sample n is zeros in sw and so in every column.  rss_all is [n_eig][P].
__global__ void __launch_bounds__(SC_THREADS)
lmm_snp_column_kernel(int64_t n_ld, int64_t pc, int64_t p0, int64_t P, int n_eig, int cz, const double *__restrict__ sw,
                      const double *__restrict__ qz, const double *__restrict__ yt, const double *__restrict__ rss0,
                      double *__restrict__ cols, double *__restrict__ rss_all) {
    const int64_t idx = (int64_t)blockIdx.x * SC_THREADS + threadIdx.x;
    if (idx >= pc * n_eig * n_ld) return;
    const int64_t pe = idx / n_ld, s = idx % n_ld, p = pe / n_eig;
    const int e = (int)(pe % n_eig);
    const double w = sw[idx];
    double *out = cols + ((int64_t)e * (cz + 2) * P + p0 + p) * n_ld + s;
    const int64_t q_stride = P * n_ld;
    out[0] = w * yt[idx];
    out[q_stride] = w * w;
    for (int k = 0; k < cz; ++k) out[(2 + k) * q_stride] = w * qz[(pe * cz + k) * n_ld + s];
    if (s == 0) rss_all[(int64_t)e * P + p0 + p] = rss0[pe];
}

// ---- the product ---------------------------------------------------------------------------------------------------------------

// One sweep over K = n_ld of a 64 x 64 tile with NB B operands beside each other: scan_snp_lod_kernel's operand maps,
// LDS stride, K chunk of 32 and prefetch; the A block is staged once per chunk and every B block q0 + u, u < NB, of the
// columns (q_stride doubles apart) has its own place in LDS and its own four accumulators.  FIRST: the operands are g, o
// and the first covariate columns, and the A operand of o is the square of the value read for g, squared in registers
// after the LDS read.  An entry's chain is the chunks in order and within a chunk the MFMAs in order: it depends on the
// SNP's row and the phenotype's column alone.  Ends with a barrier: the LDS is free for the next sweep.
template <int NB, bool FIRST>
__device__ __forceinline__ void lmm_snp_sweep(scan_d4 (&acc)[NB][4], double *lds, const double *__restrict__ xs,
                                              const double *__restrict__ bq, int64_t q_stride, int64_t n_ld, int64_t row0,
                                              int64_t rows, int64_t col0, int64_t pc) {
    double *lds_a = lds, *lds_b = lds + SC_ROWS * SC_LD;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, i = lane & 15, g = lane >> 4;
#pragma unroll
    for (int u = 0; u < NB; ++u)
#pragma unroll
        for (int t = 0; t < 4; ++t) acc[u][t] = scan_d4{0.0, 0.0, 0.0, 0.0};
    const double *ra = lds_a + (wave * 16 + i) * SC_LD + g, *rb = lds_b + i * SC_LD + g;
    auto multiply = [&]() {
#pragma unroll
        for (int kk = 0; kk < SC_KC; kk += 4) {
            const double av = ra[kk], av2 = av * av;
#pragma unroll
            for (int u = 0; u < NB; ++u) {
                const double a = FIRST && u == 1 ? av2 : av;
#pragma unroll
                for (int t = 0; t < 4; ++t)
                    acc[u][t] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, rb[(u * SC_COLS + t * 16) * SC_LD + kk], acc[u][t], 0, 0, 0);
            }
        }
    };
    const int64_t chunks = n_ld / SC_KC;       // >= 1
    double va[SC_PER], vb[NB][SC_PER];
    scan_fetch(va, xs, n_ld, row0, rows);
#pragma unroll
    for (int u = 0; u < NB; ++u) scan_fetch(vb[u], bq + u * q_stride, n_ld, col0, pc);
    for (int64_t k = 1; k < chunks; ++k) {
        scan_put(lds_a, va);
#pragma unroll
        for (int u = 0; u < NB; ++u) scan_put(lds_b + u * SC_COLS * SC_LD, vb[u]);
        __syncthreads();
        scan_fetch(va, xs + k * SC_KC, n_ld, row0, rows);
#pragma unroll
        for (int u = 0; u < NB; ++u) scan_fetch(vb[u], bq + u * q_stride + k * SC_KC, n_ld, col0, pc);
        multiply();
        __syncthreads();
    }
    scan_put(lds_a, va);
#pragma unroll
    for (int u = 0; u < NB; ++u) scan_put(lds_b + u * SC_COLS * SC_LD, vb[u]);
    __syncthreads();
    multiply();
    __syncthreads();
}

// S += qtx * qtx for the sixteen entries of a lane.
__device__ __forceinline__ void lmm_snp_fold(scan_d4 (&S)[4], const scan_d4 (&q)[4]) {
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) S[t][r] += q[t][r] * q[t][r];
}

// blockIdx.x: row tile tile0 + blockIdx.x of the SNP chunk (64 rows of xs [rows][n_ld], cut from the chunk's first SNP as
// §29 cuts them), blockIdx.y: block of 64 phenotypes of the phenotype chunk.  One launch serves the SNPs [row_lo, row_hi)
// of the chunk, a run that shares decomposition e: bq, rss0 are that decomposition's columns and null sums, offset to
// the phenotype chunk.  A tile that straddles two runs is computed once per run and stores only the run's rows, so no
// entry's chain changes: the other rows of the tile are multiplied with columns that are not theirs and are dropped.
// The first sweep accumulates b, raw and the first LS_GROUP covariate columns; every further group of covariate columns
// re-sweeps K, and S takes the squares in ascending k after each group: at cz = 16 the cz + 2 quantities of 32 VGPRs each
// would not fit the register file, at cz <= 2 there is one sweep.  The epilogue applies the test in the lane that holds the
// entry, passes LOD and flag through LDS as [column][row] and stores consecutive SNPs of one phenotype's row from
// consecutive threads.  Rows past the chunk and columns past pc shadow the last valid one and are not stored.  lod and
// used are the chunk's [pc][ld].
__global__ void __launch_bounds__(SC_THREADS)
lmm_snp_lod_kernel(int64_t rows, int64_t row_lo, int64_t row_hi, int64_t tile0, int64_t pc, int64_t n_ld, int64_t ld, int cz,
                   double half_n, const double *__restrict__ xs, const double *__restrict__ bq, int64_t q_stride,
                   const double *__restrict__ rss0, double *__restrict__ lod, uint8_t *__restrict__ used) {
    extern __shared__ __attribute__((aligned(16))) double lmm_snp_lds[];
    double *lds = lmm_snp_lds;
    const int64_t row0 = (tile0 + blockIdx.x) * SC_ROWS, col0 = (int64_t)blockIdx.y * SC_COLS;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, i = lane & 15, g = lane >> 4;
    scan_d4 b[4], raw[4], S[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) S[t] = scan_d4{0.0, 0.0, 0.0, 0.0};
    if (cz == 1) {
        scan_d4 acc[3][4];
        lmm_snp_sweep<3, true>(acc, lds, xs, bq, q_stride, n_ld, row0, rows, col0, pc);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            b[t] = acc[0][t];
            raw[t] = acc[1][t];
        }
        lmm_snp_fold(S, acc[2]);
    } else {
        scan_d4 acc[LS_MAX_B][4];
        lmm_snp_sweep<LS_MAX_B, true>(acc, lds, xs, bq, q_stride, n_ld, row0, rows, col0, pc);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            b[t] = acc[0][t];
            raw[t] = acc[1][t];
        }
#pragma unroll
        for (int u = 0; u < LS_GROUP; ++u) lmm_snp_fold(S, acc[2 + u]);
    }
    for (int k0 = LS_GROUP; k0 < cz; k0 += LS_GROUP) {
        if (cz - k0 >= LS_GROUP) {
            scan_d4 acc[LS_GROUP][4];
            lmm_snp_sweep<LS_GROUP, false>(acc, lds, xs, bq + (2 + k0) * q_stride, q_stride, n_ld, row0, rows, col0, pc);
#pragma unroll
            for (int u = 0; u < LS_GROUP; ++u) lmm_snp_fold(S, acc[u]);
        } else {
            scan_d4 acc[1][4];
            lmm_snp_sweep<1, false>(acc, lds, xs, bq + (2 + k0) * q_stride, q_stride, n_ld, row0, rows, col0, pc);
            lmm_snp_fold(S, acc[0]);
        }
    }
    static_assert(LS_GROUP == 2, "a group's remainder is one column");
    double *out_lod = lds;                                                     // [64 columns][LS_OUT_LD]
    uint8_t *out_used = reinterpret_cast<uint8_t *>(lds + SC_COLS * LS_OUT_LD);     // the same shape
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int col = t * 16 + i;
        const double r0 = rss0[std::min(col0 + col, pc - 1)];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const double G = raw[t][r] - S[t][r];
            const bool ok = G > 0.0 && G > SC_PIVOT * raw[t][r];
            const double ess = b[t][r] * b[t][r] / G;
            const int at = col * LS_OUT_LD + wave * 16 + g + 4 * r;
            out_lod[at] = ok ? scan_lod(r0, ess, half_n) : 0.0;
            out_used[at] = ok ? 1 : 0;
        }
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < SC_COLS * SC_ROWS / SC_THREADS; ++u) {
        const int idx = threadIdx.x + SC_THREADS * u, col = idx / SC_ROWS, row = idx % SC_ROWS;
        const int64_t j = row0 + row, p = col0 + col;
        if (j >= row_lo && j < row_hi && p < pc) {
            lod[p * ld + j] = out_lod[col * LS_OUT_LD + row];
            used[p * ld + j] = out_used[col * LS_OUT_LD + row];
        }
    }
}

// ---- peaks -----------------------------------------------------------------------------------------------------------------------

// scan_snp_peak_kernel with `used` per phenotype ([pc][ld]) and a count: one wavefront per (chromosome, phenotype of the
// phenotype chunk), once per SNP chunk [first, first + count).  The winner replaces what the chunks before left only when
// it is larger, and the chunk's used SNPs are added to n_used, which starts at 0; peak_index starts at -1.  No atomics.
__global__ void __launch_bounds__(64)
lmm_snp_peak_kernel(int64_t first, int64_t count, int64_t ld, int n_chrom, const int64_t *__restrict__ snp_off,
                    const uint8_t *__restrict__ used, const double *__restrict__ lod, double *__restrict__ peak_lod,
                    int64_t *__restrict__ peak_index, int64_t *__restrict__ n_used) {
    const int c = blockIdx.x;
    const int64_t p = blockIdx.y, lo = std::max(snp_off[c], first), hi = std::min(snp_off[c + 1], first + count);
    double best = -__builtin_huge_val();
    int64_t at = -1;
    long long seen = 0;
    for (int64_t j = lo + threadIdx.x; j < hi; j += 64) {
        if (!used[p * ld + (j - first)]) continue;
        ++seen;
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
        seen += __shfl_xor(seen, off, WAVE);
        if (oa >= 0 && (at < 0 || ov > best || (ov == best && oa < at))) {
            best = ov;
            at = oa;
        }
    }
    if (threadIdx.x == 0 && at >= 0) {
        const int64_t slot = p * n_chrom + c;
        n_used[slot] += seen;
        if (peak_index[slot] < 0 || best > peak_lod[slot]) {
            peak_lod[slot] = best;
            peak_index[slot] = at;
        }
    }
}
