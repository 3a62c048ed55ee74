// Genome scan (gbrs_scan_*): Haley-Knott regression of phenotypes on the founder dosages of a cohort at
// every grid point, with additive covariates.  gfx950 only.
//
// prepare: one workgroup per grid point turns the point's dosage columns into W_m = L^-1 X~' (scan_prepare_kernel), so
// that the explained sum of squares of a phenotype at the point is |W_m y~|^2.  run: the phenotypes are projected and
// transposed (scan_pheno_kernel), and one product kernel (scan_lod_kernel) multiplies W [M Hp][n_ld] with the phenotype
// block [P][n_ld] on v_mfma_f64_16x16x4_f64, squares and sums the Hp rows of every grid point in its epilogue and stores
// LODs only.  Both operands are row-major with the sample axis (K) contiguous and zero filled up to n_ld, a multiple of
// the K chunk: the operand maps, the LDS stride and the prefetch are those of match_cross_kernel (hmm_match.inc), without
// its K tail and its 8-byte staging.  permute (kernels in scan_perm.inc): permutations of the projected
// phenotypes, drawn and gathered on the device, pass through the same product and peak kernels as further columns, and
// one maximum per (phenotype, permutation) comes back.  SNP association (kernels and the rule in
// scan_snp.inc): a row kernel builds one normalised row per founder SNP from two grid points and a bit pattern, and a
// sibling of the product kernel with one row per SNP turns the rows into LODs.  Mediation (kernels and the
// rule in scan_mediate.inc): a sibling of the product kernel gathers the W rows of each target's point, multiplies them
// with the projected mediators and applies the conditional regression's rule in its epilogue.  Founder effects and LOD
// support intervals (kernels and the rules in scan_effects.inc): one workgroup per peak forms the founder
// effects and their standard errors from W_m and the point's dosage columns, and one wavefront per (chromosome,
// phenotype) walks outward from the peak over the chunk's LOD rows while they are on the device.  Linear mixed model
// (kernels and the rule in scan_lmm.inc): the kinship of the cohort per chromosome, the rotation of the
// cohort by a kinship's eigenvectors, the REML fit of every phenotype's heritability and a weighted scan that forms each
// (grid point, phenotype) pair's explained sum of squares without a W.  SNP association under the mixed model (DESIGN.md §33;
// kernels and the rule in scan_lmm_snp.inc): the SNP dosages of §29 rotated as the cohort is, and a sibling of the SNP product
// kernel that multiplies them with the weighted columns of every phenotype's null fit and applies the test in its epilogue.
// Interactive covariates (kernels and the rule in scan_int.inc): a preparation of its own that factors a point's
// additive columns and then their products with the interactive covariates, and a sibling of the product kernel whose
// epilogue gives the LODs of the full model, of the additive model and of the interaction from one product.
#include "common.h"
#include "scan_hmm.h"

#include <algorithm>
#include <cmath>
#include <limits>

namespace gbrs {

typedef double scan_d4 __attribute__((ext_vector_type(4)));

constexpr int SC_ROWS = 64, SC_COLS = 64, SC_KC = 32, SC_LD = SC_KC + 2, SC_THREADS = 256;
constexpr int SC_PER = SC_ROWS * SC_KC / SC_THREADS;
constexpr int SC_MAX_C = 64;               // covariate columns, intercept included
constexpr int64_t SC_PCHUNK = 512;         // phenotype columns on the device at a time
constexpr double SC_PIVOT = 1e-10;         // the skip rule's threshold: d_j > SC_PIVOT * G_jj
static_assert(SC_LD % 32 == 2 && SC_KC % 4 == 0, "the bank argument of match_cross_kernel");
static_assert(SC_ROWS == 16 * (SC_THREADS / 64) && SC_COLS == 64 && SC_PCHUNK % SC_COLS == 0, "tile shape");

// ---- prepare ----------------------------------------------------------------------------------------------------------------

// One workgroup per grid point m; the point's Hp rows of W are its workspace.  Every sum over the samples is formed by
// one wavefront, lane l adding the samples l, l + 64, ... in order and the 64 partial sums meeting in a butterfly: the
// order depends on n alone.  The factorisation is one thread's, in the column order of the rule.
//   1  w[j][s] = D[s][m][j] for the H - 1 kept founders, zeros in the padding rows and past sample n
//   2  qtx[k][j] = sum_s qz[s][k] w[j][s], raw[j] = sum_s w[j][s]^2
//   3  w[j][s] -= sum_k qz[s][k] qtx[k][j]                  (X~, transposed)
//   4  G[j][i] = sum_s w[j][s] w[i][s], i <= j
//   5  Cholesky with the skip rule -> L, keep[], rank[m].  The covariates are the columns before column 0: a column that
//      the projection took to rounding (G_jj <= SC_PIVOT raw[j]) counts as G_jj = 0, by the rule's own threshold
//   6  per sample, forward substitution down the kept columns: w[j][s] = (w[j][s] - sum_{kept i<j} L[j][i] w[i][s]) / L[j][j]
template <int HP>
__global__ void __launch_bounds__(SC_THREADS)
scan_prepare_kernel(int n, int64_t M, int H, int c, int64_t n_ld, const double *__restrict__ D, const double *__restrict__ qz,
                    double *__restrict__ W, int32_t *__restrict__ rank) {
    __shared__ double qtx[SC_MAX_C * HP];
    __shared__ double G[HP * HP], L[HP * HP], raw[HP];
    __shared__ int keep[HP];
    const int64_t m = blockIdx.x;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, Hx = H - 1;
    double *w = W + m * HP * n_ld;
    for (int idx = tid; idx < n * Hx; idx += SC_THREADS) {
        const int s = idx / Hx, j = idx % Hx;
        w[j * n_ld + s] = D[((int64_t)s * M + m) * H + j];
    }
    for (int64_t idx = tid; idx < HP * n_ld; idx += SC_THREADS)
        if (idx / n_ld >= Hx || idx % n_ld >= n) w[idx] = 0.0;
    __syncthreads();
    for (int q = wave; q < (c + 1) * Hx; q += SC_THREADS / 64) {
        const int k = q / Hx, j = q % Hx;
        double acc = 0.0;
        if (k < c)
            for (int s = lane; s < n; s += 64) acc += qz[(int64_t)s * c + k] * w[j * n_ld + s];
        else
            for (int s = lane; s < n; s += 64) acc += w[j * n_ld + s] * w[j * n_ld + s];
        acc = wave_sum_all(acc);
        if (lane == 0) (k < c ? qtx[k * HP + j] : raw[j]) = acc;
    }
    __syncthreads();
    for (int idx = tid; idx < n * Hx; idx += SC_THREADS) {
        const int j = idx / n, s = idx % n;
        double p = 0.0;
        for (int k = 0; k < c; ++k) p += qz[(int64_t)s * c + k] * qtx[k * HP + j];
        w[j * n_ld + s] -= p;
    }
    __syncthreads();
    for (int q = wave; q < Hx * (Hx + 1) / 2; q += SC_THREADS / 64) {
        int j = 0;
        while ((j + 1) * (j + 2) / 2 <= q) ++j;
        const int i = q - j * (j + 1) / 2;
        double acc = 0.0;
        for (int s = lane; s < n; s += 64) acc += w[j * n_ld + s] * w[i * n_ld + s];
        acc = wave_sum_all(acc);
        if (lane == 0) G[j * HP + i] = acc;
    }
    __syncthreads();
    if (tid == 0) {
        int kept = 0;
        for (int j = 0; j < Hx; ++j) {
            const double gjj = G[j * HP + j];
            double d = gjj;
            for (int i = 0; i < j; ++i) {
                double v = 0.0;
                if (keep[i]) {
                    v = G[j * HP + i];
                    for (int k = 0; k < i; ++k)
                        if (keep[k]) v -= L[j * HP + k] * L[i * HP + k];
                    v /= L[i * HP + i];
                    d -= v * v;
                }
                L[j * HP + i] = v;
            }
            const int ok = gjj > SC_PIVOT * raw[j] && d > SC_PIVOT * gjj;
            keep[j] = ok;
            kept += ok;
            if (ok) L[j * HP + j] = sqrt(d);
            else
                for (int i = 0; i <= j; ++i) L[j * HP + i] = 0.0;
        }
        rank[m] = kept;
    }
    __syncthreads();
    for (int s = tid; s < n; s += SC_THREADS) {
        double x[HP];
#pragma unroll
        for (int j = 0; j < HP; ++j) {
            double v = 0.0;
            if (j < Hx && keep[j]) {
                v = w[j * n_ld + s];
#pragma unroll
                for (int i = 0; i < j; ++i)
                    if (keep[i]) v -= L[j * HP + i] * x[i];
                v /= L[j * HP + j];
            }
            x[j] = v;
            if (j < Hx) w[j * n_ld + s] = v;
        }
    }
}

// ---- phenotypes --------------------------------------------------------------------------------------------------------------

// One wavefront per phenotype of the chunk: y~ = y - qz qz' y into row p of yt ([columns][n_ld], zeros past sample n) and
// rss0[p] = |y~|^2, the sums in the order of scan_prepare_kernel's.  y is [n][ld_y], the chunk's columns of the upload.
__global__ void __launch_bounds__(64)
scan_pheno_kernel(int n, int c, int64_t n_ld, int64_t ld_y, const double *__restrict__ y, const double *__restrict__ qz,
                  double *__restrict__ yt, double *__restrict__ rss0) {
    __shared__ double qty[SC_MAX_C];
    const int64_t p = blockIdx.x;
    const int lane = threadIdx.x;
    for (int k = 0; k < c; ++k) {
        double acc = 0.0;
        for (int s = lane; s < n; s += 64) acc += qz[(int64_t)s * c + k] * y[(int64_t)s * ld_y + p];
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
            v = y[s * ld_y + p] - proj;
        }
        yt[p * n_ld + s] = v;
        ss += v * v;
    }
    ss = wave_sum_all(ss);
    if (lane == 0) rss0[p] = ss;
}

// ---- the product -------------------------------------------------------------------------------------------------------------

// One 64 x SC_KC operand block on its way to LDS: sixteen lanes across the 256 contiguous bytes of a row, one aligned
// 16-byte load and one 16-byte LDS store per pair of columns.  Rows past the last one shadow it.
__device__ __forceinline__ void scan_fetch(double (&v)[SC_PER], const double *__restrict__ src, int64_t ld, int64_t first,
                                           int64_t n_rows) {
    const int t = threadIdx.x;
#pragma unroll
    for (int i = 0; i < SC_PER / 2; ++i) {
        const int idx = t + SC_THREADS * i, r = idx / (SC_KC / 2), k = 2 * (idx % (SC_KC / 2));
        const double2 x = *reinterpret_cast<const double2 *>(src + std::min(first + r, n_rows - 1) * ld + k);
        v[2 * i] = x.x;
        v[2 * i + 1] = x.y;
    }
}

__device__ __forceinline__ void scan_put(double *dst, const double (&v)[SC_PER]) {
    const int t = threadIdx.x;
#pragma unroll
    for (int i = 0; i < SC_PER / 2; ++i) {
        const int idx = t + SC_THREADS * i, r = idx / (SC_KC / 2), k = 2 * (idx % (SC_KC / 2));
        *reinterpret_cast<double2 *>(dst + r * SC_LD + k) = double2{v[2 * i], v[2 * i + 1]};
    }
}

__device__ __forceinline__ double scan_lod(double rss0, double ess, double half_n) {
    if (rss0 == 0.0) return 0.0;
    const double rss1 = rss0 - ess;
    if (rss1 <= 0.0) return __builtin_huge_val();
    return half_n * log10(rss0 / rss1);
}

// blockIdx.x: block of 64 rows of W = 64 / HP grid points (fastest, so the row blocks that share a phenotype block run side
// by side), blockIdx.y: block of 64 phenotypes of the chunk.  Wavefront w multiplies rows 16 w .. 16 w + 15 with the 64
// columns: four 16x16 accumulators, register r of lane (g = lane >> 4, i = lane & 15) is row g + 4 r, column 16 t + i.
// K = n_ld is one chain of MFMAs per accumulator, chunk after chunk, not split and without atomics; the loads of chunk
// k + 1 are in flight during the MFMAs of chunk k.
// Epilogue: a grid point's HP rows lie within one wavefront's 16.  At HP = 8 the registers 0, 1 of a lane are rows of the
// wavefront's first point and 2, 3 of its second; at HP = 16 all four are the one point's.  Squares are added in the lane
// in register order, then across the four lane groups (xor 16, xor 32: a fixed tree), so ess depends on nothing but the
// rows and the column.  ess goes to LDS as [column][point]; every thread then turns two of the 64 x 64 / HP values into
// LODs and stores them, consecutive threads consecutive grid points of one phenotype's row.  Rows past M HP and columns
// past P shadow the last valid one and are not stored.  lod is the chunk's [P][M].
template <int HP>
__global__ void __launch_bounds__(SC_THREADS)
scan_lod_kernel(int64_t M, int64_t P, int64_t n_ld, double half_n, const double *__restrict__ W, const double *__restrict__ yt,
                const double *__restrict__ rss0, double *__restrict__ lod) {
    constexpr int PTS = SC_ROWS / HP, PPW = 16 / HP;      // grid points per workgroup and per wavefront
    __shared__ __attribute__((aligned(16))) double lds_a[SC_ROWS * SC_LD];
    __shared__ __attribute__((aligned(16))) double lds_b[SC_COLS * SC_LD];
    const int64_t row0 = (int64_t)blockIdx.x * SC_ROWS, col0 = (int64_t)blockIdx.y * SC_COLS, rows = M * HP;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, i = lane & 15, g = lane >> 4;
    scan_d4 acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = scan_d4{0.0, 0.0, 0.0, 0.0};
    const double *ra = lds_a + (wave * 16 + i) * SC_LD + g, *rb = lds_b + i * SC_LD + g;
    auto multiply = [&]() {
#pragma unroll
        for (int kk = 0; kk < SC_KC; kk += 4) {
            const double av = ra[kk];
#pragma unroll
            for (int t = 0; t < 4; ++t) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, rb[t * 16 * SC_LD + kk], acc[t], 0, 0, 0);
        }
    };
    const int64_t chunks = n_ld / SC_KC;       // >= 1
    double va[SC_PER], vb[SC_PER];
    scan_fetch(va, W, n_ld, row0, rows);
    scan_fetch(vb, yt, n_ld, col0, P);
    for (int64_t k = 1; k < chunks; ++k) {
        scan_put(lds_a, va);
        scan_put(lds_b, vb);
        __syncthreads();
        scan_fetch(va, W + k * SC_KC, n_ld, row0, rows);
        scan_fetch(vb, yt + k * SC_KC, n_ld, col0, P);
        multiply();
        __syncthreads();
    }
    scan_put(lds_a, va);
    scan_put(lds_b, vb);
    __syncthreads();
    multiply();
    __syncthreads();
    double *ess = lds_a;                       // [64 columns][PTS]
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        double e[PPW];
        if constexpr (HP == 8) {
            e[0] = acc[t][0] * acc[t][0] + acc[t][1] * acc[t][1];
            e[1] = acc[t][2] * acc[t][2] + acc[t][3] * acc[t][3];
        } else {
            e[0] = ((acc[t][0] * acc[t][0] + acc[t][1] * acc[t][1]) + acc[t][2] * acc[t][2]) + acc[t][3] * acc[t][3];
        }
#pragma unroll
        for (int q = 0; q < PPW; ++q) {
            e[q] += __shfl_xor(e[q], 16, WAVE);
            e[q] += __shfl_xor(e[q], 32, WAVE);
            if (g == 0) ess[(t * 16 + i) * PTS + wave * PPW + q] = e[q];
        }
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < SC_COLS * PTS / SC_THREADS; ++u) {
        const int idx = threadIdx.x + SC_THREADS * u, col = idx / PTS, pt = idx % PTS;
        const int64_t m = (int64_t)blockIdx.x * PTS + pt, p = col0 + col;
        if (m < M && p < P) lod[p * M + m] = scan_lod(rss0[p], ess[idx], half_n);
    }
}

// ---- peaks -------------------------------------------------------------------------------------------------------------------

// One wavefront per (chromosome, phenotype of the chunk): lane l looks at the chromosome's points l, l + 64, ... in order
// and keeps the first of its largest; the 64 candidates meet in a butterfly that prefers the larger value and, among
// equal ones, the lower index.  No atomics.  A chromosome without points gives NaN and -1.
__global__ void __launch_bounds__(64)
scan_peak_kernel(int64_t M, int n_chrom, const int64_t *__restrict__ point_off, const double *__restrict__ lod,
                 double *__restrict__ peak_lod, int64_t *__restrict__ peak_index) {
    const int c = blockIdx.x;
    const int64_t p = blockIdx.y, lo = point_off[c], hi = point_off[c + 1];
    double best = -__builtin_huge_val();
    int64_t at = -1;
    for (int64_t m = lo + threadIdx.x; m < hi; m += 64) {
        const double v = lod[p * M + m];
        if (at < 0 || v > best) {
            best = v;
            at = m;
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
    if (threadIdx.x == 0) {
        peak_lod[p * n_chrom + c] = at < 0 ? __builtin_nan("") : best;
        peak_index[p * n_chrom + c] = at;
    }
}

// ---- permutation thresholds ----------------------------------------------------------------------------------------------------

#include "philox.h"
#include "scan_perm.inc"

// ---- SNP association ---------------------------------------------------------------------------------------------------------

#include "scan_snp.inc"

// ---- mediation ---------------------------------------------------------------------------------------------------------------

#include "scan_mediate.inc"

// ---- founder effects and support intervals -------------------------------------------------------------------------------------

#include "scan_effects.inc"

// ---- linear mixed model --------------------------------------------------------------------------------------------------------

#include "scan_lmm.inc"

// ---- SNP association under the mixed model -------------------------------------------------------------------------------------

#include "scan_lmm_snp.inc"

// ---- founder effects under the mixed model -------------------------------------------------------------------------------------

#include "scan_lmm_effects.inc"

// ---- interactive covariates ----------------------------------------------------------------------------------------------------

#include "scan_int.inc"

}  // namespace gbrs

using namespace gbrs;

// The handle: the grid, then one group per feature.  A group owns its device buffers, sums them in bytes() and drops what
// an append invalidates in unprepare(); `last` holds the report of every pass as the public struct itself.
struct gbrs_scan {
    int device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    int n_chrom = 0, H = 0, Hp = 0;
    int64_t M = 0;
    std::vector<int32_t> points;              // per chromosome
    std::vector<int64_t> point_off;           // n_chrom + 1
    DevBuf<int64_t> d_point_off;
    // the cohort: [capacity][M][H], the first n rows in use
    struct Cohort {
        int64_t n = 0, capacity = 0;
        DevBuf<double> dosage;
    } cohort;
    // what gbrs_scan_prepare made (c 0: not prepared), and one chunk of gbrs_scan_run
    struct Prep {
        int c = 0;
        int64_t n_ld = 0;
        DevBuf<double> qz, W;
        DevBuf<int32_t> d_rank;
        std::vector<int32_t> rank;
        DevBuf<double> y, yt, rss0, lod, peak_lod;
        DevBuf<int64_t> peak_index;
        uint64_t bytes() const {
            return qz.bytes() + W.bytes() + d_rank.bytes() + y.bytes() + yt.bytes() + rss0.bytes() + lod.bytes() + peak_lod.bytes() +
                   peak_index.bytes();
        }
        void unprepare() {
            c = 0;
            rank.clear();
        }
    } prep;
    // the SNPs of gbrs_scan_set_snps in handle order (chromosome after chromosome): SS_TABLE_BYTES per SNP
    struct Snp {
        int64_t M = 0;
        std::vector<int64_t> off;             // n_chrom + 1
        DevBuf<int64_t> d_off;
        DevBuf<int32_t> lo, hi;               // global point indices
        DevBuf<uint32_t> mask;
        DevBuf<double> t;
        uint64_t bytes() const { return d_off.bytes() + lo.bytes() + hi.bytes() + mask.bytes() + t.bytes(); }
        void clear() {
            M = 0;
            off.clear();
            d_off.release();
            lo.release();
            hi.release();
            mask.release();
            t.release();
        }
    } snp;
    // the per-chromosome products S_c of gbrs_scan_kinship, [n_chrom][n][n]: kept until the next append
    struct Kin {
        DevBuf<double> S;
        bool valid = false;
    } kin;
    // what gbrs_scan_lmm_prepare made (cz 0: not prepared): the decompositions, the rotated covariates [n_eig][cz][n_ld]
    // and the rotated cohort [M][Hp][n_ld]; the ranks are the last gbrs_scan_lmm_run's
    struct Lmm {
        int cz = 0, n_eig = 0;
        int64_t n_ld = 0;
        DevBuf<double> U, lam, Zs, R;
        DevBuf<int32_t> eig_of_point;
        std::vector<int32_t> eig_of_chrom, rank_min, rank_max;
        uint64_t bytes() const { return U.bytes() + lam.bytes() + Zs.bytes() + R.bytes() + eig_of_point.bytes(); }
        void unprepare() {
            cz = 0;
            n_eig = 0;
        }
    } lmm;
    // what gbrs_scan_int_prepare made (c 0: not prepared): its own qz, the interactive covariates and the W of §35,
    // [M * hpi][n_ld]; the ranks are [2][M] on the device, full then additive
    struct Inter {
        int c = 0, k = 0, hpi = 0;
        int64_t n_ld = 0;
        DevBuf<double> qz, zint, W;
        DevBuf<int32_t> d_rank;
        std::vector<int32_t> rank_full, rank_add;
        uint64_t bytes() const { return qz.bytes() + zint.bytes() + W.bytes() + d_rank.bytes(); }
        void unprepare() {                    // its W included
            c = 0;
            k = 0;
            hpi = 0;
            rank_full.clear();
            rank_add.clear();
            W.release();
        }
    } inter;
    // The reports: a pass fills the fields of its own when it has succeeded, its getter adds the few that are read live.
    // The buffers of a pass are the call's own and are gone when it returns.
    struct Last {
        gbrs_scan_info_t scan = {};
        gbrs_scan_perm_info_t perm = {};
        gbrs_scan_snp_info_t snp = {};
        gbrs_scan_mediate_info_t mediate = {};
        gbrs_scan_effects_info_t effects = {};
        gbrs_scan_lmm_info_t lmm = {};
        gbrs_scan_lmm_snp_info_t lmm_snp = {};
        gbrs_scan_lmm_effects_info_t lmm_effects = {};
        gbrs_scan_int_info_t inter = {};
    } last;
    // gbrs_scan_info_t's figure: the grid, the cohort, the preparation and gbrs_scan_run's chunk
    uint64_t scan_bytes() const { return d_point_off.bytes() + cohort.dosage.bytes() + prep.bytes(); }
    // every buffer the handle owns, whatever is prepared: with a pass's own buffers, its peak_device_bytes
    uint64_t resident_bytes() const { return scan_bytes() + snp.bytes() + kin.S.bytes() + lmm.bytes() + inter.bytes(); }
};

namespace {

// ---- what the passes do around their kernels -----------------------------------------------------------------
// The checks are steps, not one call: the passes put their own checks between them, and the first error counts.

// a table [n][cols] of the samples' values: `noun` is "phenotype", "target" or "mediator"
int check_finite(const char *noun, const double *table, int64_t n, int64_t cols) {
    for (int64_t k = 0; k < n * cols; ++k)
        if (!std::isfinite(table[k]))
            return fail(GBRS_ERR_INVALID, "%s %lld holds a value that is not finite (sample %lld)", noun, (long long)(k % cols),
                        (long long)(k / cols));
    return GBRS_OK;
}

// the heritabilities a caller gives, [P][n_eig], nullable
int check_hsq(const double *hsq_in, int64_t P, int n_eig) {
    if (hsq_in)
        for (int64_t k = 0; k < P * n_eig; ++k)
            if (!(hsq_in[k] >= 0.0 && hsq_in[k] <= 1.0))
                return fail(GBRS_ERR_INVALID, "the heritability given for phenotype %lld and decomposition %d is %g, outside [0, 1]",
                            (long long)(k / n_eig), (int)(k % n_eig), hsq_in[k]);
    return GBRS_OK;
}

// the targets of a pass: a column of [0, P) (where the pass has columns) and a grid point each
int check_targets(const gbrs_scan *s, int64_t T, const int64_t *column, int64_t P, const int64_t *point) {
    for (int64_t t = 0; t < T; ++t) {
        if (column && (column[t] < 0 || column[t] >= P))
            return fail(GBRS_ERR_INVALID, "target %lld is phenotype column %lld: the table has the columns 0 .. %lld", (long long)t,
                        (long long)column[t], (long long)(P - 1));
        if (point[t] < 0 || point[t] >= s->M)
            return fail(GBRS_ERR_INVALID, "target %lld is at grid point %lld: the handle has the points 0 .. %lld", (long long)t,
                        (long long)point[t], (long long)(s->M - 1));
    }
    return GBRS_OK;
}

// the sample axis of every product operand: zero filled up to a multiple of the K chunk
int64_t padded(int64_t n) { return (n + SC_KC - 1) / SC_KC * SC_KC; }

// The buffers a pass allocates for itself go through its tally: resident_bytes() + own.bytes is the pass's peak, and a
// buffer that only some calls need counts when it is there.
struct Tally {
    uint64_t bytes = 0;
    template <typename T>
    int alloc(DevBuf<T> &buf, size_t count) {
        GBRS_TRY(buf.alloc(count));
        bytes += buf.bytes();
        return GBRS_OK;
    }
};

// columns [col0, col0 + pc) of the host table [n][ld] to y [n][pc], on the handle's stream
int upload_columns(gbrs_scan *s, DevBuf<double> &y, const double *table, int64_t ld, int64_t col0, int64_t pc) {
    GBRS_HIP_CHECK(hipMemcpy2DAsync(y.p, (size_t)pc * sizeof(double), table + col0, (size_t)ld * sizeof(double),
                                    (size_t)pc * sizeof(double), (size_t)s->cohort.n, hipMemcpyHostToDevice, s->stream));
    return GBRS_OK;
}

// those columns with the covariates qz [n][c] projected out, transposed to yt [pc][n_ld], and their sums of squares to rss
int project(gbrs_scan *s, const DevBuf<double> &qz, int c, int64_t n_ld, const double *table, int64_t ld, int64_t col0, int64_t pc,
            DevBuf<double> &y, double *yt, double *rss) {
    GBRS_TRY(upload_columns(s, y, table, ld, col0, pc));
    hipLaunchKernelGGL(scan_pheno_kernel, dim3((unsigned)pc), dim3(64), 0, s->stream, (int)s->cohort.n, c, n_ld, pc, y.p, qz.p, yt, rss);
    return GBRS_OK;
}

// y~ of every column of the table [n][P], by gbrs_scan_run's kernel in gbrs_scan_run's chunks: it stays on the device for
// the pass as yt_all [P][n_ld] and rss_all [P]
int project_all(gbrs_scan *s, const DevBuf<double> &qz, int c, int64_t n_ld, const double *table, int64_t P, DevBuf<double> &y,
                DevBuf<double> &yt_all, DevBuf<double> &rss_all) {
    for (int64_t p0 = 0; p0 < P; p0 += SC_PCHUNK) {
        GBRS_TRY(project(s, qz, c, n_ld, table, P, p0, std::min(SC_PCHUNK, P - p0), y, yt_all.p + p0 * n_ld, rss_all.p + p0));
        GBRS_HIP_CHECK(hipGetLastError());
    }
    return GBRS_OK;
}

// The pass-wide timed region of the handle's stream opens with a record of ev[0] ...
int timed_open(gbrs_scan *s) {
    GBRS_HIP_CHECK(hipEventRecord(s->ev[0], s->stream));
    return GBRS_OK;
}

// ... and this closes it with ev[1] and waits for it.
int timed_wait(gbrs_scan *s) {
    GBRS_HIP_CHECK(hipEventRecord(s->ev[1], s->stream));
    GBRS_HIP_CHECK(hipGetLastError());
    GBRS_HIP_CHECK(hipStreamSynchronize(s->stream));
    return GBRS_OK;
}

// device milliseconds between two events that were waited for; `unread` (0.0, or the time to keep) where they cannot be read
double elapsed_ms(hipEvent_t from, hipEvent_t to, double unread) {
    float ms = 0.f;
    return hipEventElapsedTime(&ms, from, to) == hipSuccess ? ms : unread;
}

// the region of the handle's ev[0] and ev[1]
double pass_ms(const gbrs_scan *s, double unread) { return elapsed_ms(s->ev[0], s->ev[1], unread); }

// a few events of a call's own, for the parts of a chunk that a pass times where it waits for the chunk anyway
struct Marks {
    hipEvent_t ev[4] = {};
    ~Marks() {
        for (auto e : ev)
            if (e) (void)hipEventDestroy(e);
    }
    int create() {
        for (auto &e : ev) GBRS_HIP_CHECK(hipEventCreate(&e));
        return GBRS_OK;
    }
};

// Pairs of events around the product kernel of consecutive chunks, so that a pass times it without waiting per chunk: a
// pair is read when its turn comes round again, and the rest after the pass.
struct EventRing {
    static constexpr int PAIRS = 8;
    hipEvent_t ev[2 * PAIRS] = {};
    int64_t used = 0;
    double ms = 0.0;
    ~EventRing() {
        for (auto e : ev)
            if (e) (void)hipEventDestroy(e);
    }
    int create() {
        for (auto &e : ev) GBRS_HIP_CHECK(hipEventCreate(&e));
        return GBRS_OK;
    }
    int read(int slot) {
        float t = 0.f;
        GBRS_HIP_CHECK(hipEventSynchronize(ev[2 * slot + 1]));
        if (hipEventElapsedTime(&t, ev[2 * slot], ev[2 * slot + 1]) == hipSuccess) ms += t;
        return GBRS_OK;
    }
    int next(int *slot) {           // the slot of the next chunk, its earlier use read
        *slot = (int)(used % PAIRS);
        if (used >= PAIRS) GBRS_TRY(read(*slot));
        ++used;
        return GBRS_OK;
    }
    int drain() {                   // after the stream was waited for
        for (int64_t k = std::max<int64_t>(0, used - PAIRS); k < used; ++k) GBRS_TRY(read((int)(k % PAIRS)));
        return GBRS_OK;
    }
};

// the first `count` elements of a result to the caller's array from element `at` on, where the caller asked for it
template <typename T>
int copy_out(T *dst, const DevBuf<T> &buf, size_t count, size_t at = 0) {
    if (dst) GBRS_HIP_CHECK(hipMemcpy(dst + at, buf.p, count * sizeof(T), hipMemcpyDeviceToHost));
    return GBRS_OK;
}

// The peaks of a SNP pass, [P][n_chrom], after the stream was waited for: NaN where a chromosome had no SNP in use.
int snp_peaks_out(const DevBuf<double> &d_peak, const DevBuf<int64_t> &d_index, double *peak_lod, int64_t *peak_index) {
    std::vector<double> h_peak(d_peak.n);
    std::vector<int64_t> h_index(d_index.n);
    GBRS_TRY(copy_out(h_peak.data(), d_peak, d_peak.n));
    GBRS_TRY(copy_out(h_index.data(), d_index, d_index.n));
    for (size_t k = 0; k < h_peak.size(); ++k)
        if (h_index[k] < 0) h_peak[k] = std::numeric_limits<double>::quiet_NaN();
    if (peak_lod) std::memcpy(peak_lod, h_peak.data(), h_peak.size() * sizeof(double));
    if (peak_index) std::memcpy(peak_index, h_index.data(), h_index.size() * sizeof(int64_t));
    return GBRS_OK;
}

// Room for `more` samples after the n in use; the samples in use move with the buffer.
int scan_reserve(gbrs_scan *s, int64_t more) {
    gbrs_scan::Cohort &co = s->cohort;
    if (co.n + more <= co.capacity) return GBRS_OK;
    const int64_t want = std::max(co.n + more, 2 * co.capacity);
    const size_t row = (size_t)s->M * s->H;
    DevBuf<double> grown;
    GBRS_TRY(grown.alloc((size_t)want * row));
    if (co.n > 0) {        // on the handle's stream and waited for: a device-to-device hipMemcpy need not be done when it returns
        GBRS_HIP_CHECK(hipMemcpyAsync(grown.p, co.dosage.p, (size_t)co.n * row * sizeof(double), hipMemcpyDeviceToDevice, s->stream));
        GBRS_HIP_CHECK(hipStreamSynchronize(s->stream));
    }
    co.dosage.swap(grown);
    co.capacity = want;
    return GBRS_OK;
}

// `count` samples were copied behind the cohort: they count, and what was made from the cohort before them is dropped -
// W, the kinship products with what gbrs_scan_lmm_prepare made, and what gbrs_scan_int_prepare made
void scan_appended(gbrs_scan *s, int64_t count) {
    s->cohort.n += count;
    s->prep.unprepare();
    s->lmm.unprepare();
    s->kin.valid = false;
    s->kin.S.release();
    s->inter.unprepare();
}

}  // namespace

extern "C" {

int gbrs_scan_create(int device, int n_chrom, const int32_t *points_per_chrom, int num_haps, gbrs_scan_t **out) {
    if (!out) return fail(GBRS_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (num_haps < 2) return fail(GBRS_ERR_INVALID, "a scan needs at least 2 founders, got %d: the last one is dropped from the design", num_haps);
    if (num_haps > 17) return fail(GBRS_ERR_INVALID, "a scan takes at most 17 founders, got %d", num_haps);
    if (n_chrom < 1 || !points_per_chrom) return fail(GBRS_ERR_INVALID, "bad argument");
    int64_t M = 0;
    for (int c = 0; c < n_chrom; ++c) {
        if (points_per_chrom[c] < 0) return fail(GBRS_ERR_INVALID, "chromosome %d has a negative number of grid points", c);
        M += points_per_chrom[c];
    }
    if (M == 0) return fail(GBRS_ERR_INVALID, "the grid has no points");
    if (M > std::numeric_limits<int32_t>::max()) return fail(GBRS_ERR_INVALID, "too many grid points");     // one workgroup per point
    GBRS_TRY(select_device(device));
    gbrs_scan *s = new gbrs_scan;
    s->device = device;
    s->n_chrom = n_chrom;
    s->H = num_haps;
    s->Hp = num_haps <= 9 ? 8 : 16;
    s->M = M;
    s->points.assign(points_per_chrom, points_per_chrom + n_chrom);
    s->point_off.assign(n_chrom + 1, 0);
    for (int c = 0; c < n_chrom; ++c) s->point_off[c + 1] = s->point_off[c] + points_per_chrom[c];
    auto build = [&]() -> int {
        GBRS_HIP_CHECK(hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking));
        for (auto &e : s->ev) GBRS_HIP_CHECK(hipEventCreate(&e));
        GBRS_TRY(s->d_point_off.alloc(s->point_off.size()));
        GBRS_HIP_CHECK(hipMemcpy(s->d_point_off.p, s->point_off.data(), s->d_point_off.bytes(), hipMemcpyHostToDevice));
        return GBRS_OK;
    };
    const int status = build();
    if (status != GBRS_OK) {
        gbrs_scan_destroy(s);
        return status;
    }
    *out = s;
    return GBRS_OK;
}

int gbrs_scan_destroy(gbrs_scan_t *s) {
    if (!s) return GBRS_OK;
    (void)hipSetDevice(s->device);
    if (s->stream) (void)hipStreamSynchronize(s->stream);
    for (auto &e : s->ev)
        if (e) (void)hipEventDestroy(e);
    if (s->stream) (void)hipStreamDestroy(s->stream);
    delete s;
    return GBRS_OK;
}

int gbrs_scan_append(gbrs_scan_t *s, int n, const double *dosage) {
    RoctxRange roctx_range("gbrs_scan_append");
    if (!s) return fail(GBRS_ERR_INVALID, "handle is NULL");
    if (n < 0 || (n > 0 && !dosage)) return fail(GBRS_ERR_INVALID, "bad argument");
    if (n == 0) return GBRS_OK;
    if (s->cohort.n + n > std::numeric_limits<int32_t>::max() / 16) return fail(GBRS_ERR_INVALID, "too many samples");
    const size_t row = (size_t)s->M * s->H;
    for (size_t k = 0; k < (size_t)n * row; ++k)
        if (!std::isfinite(dosage[k]))
            return fail(GBRS_ERR_INVALID, "dosage of sample %lld holds a value that is not finite (grid point %lld, founder %d)",
                        (long long)(s->cohort.n + (int64_t)(k / row)), (long long)(k % row / s->H), (int)(k % s->H));
    GBRS_TRY(select_device(s->device));
    GBRS_TRY(scan_reserve(s, n));
    GBRS_HIP_CHECK(hipMemcpy(s->cohort.dosage.p + (size_t)s->cohort.n * row, dosage, (size_t)n * row * sizeof(double), hipMemcpyHostToDevice));
    scan_appended(s, n);
    return GBRS_OK;
}

int gbrs_scan_append_hmm(gbrs_scan_t *s, gbrs_hmm_t *hmm, int sample) {
    RoctxRange roctx_range("gbrs_scan_append_hmm");
    if (!s) return fail(GBRS_ERR_INVALID, "handle is NULL");
    HmmGridView view;
    GBRS_TRY(hmm_grid_view(hmm, sample, &view, false));      // what the handle holds, checked before anything runs on it
    if (view.device != s->device) return fail(GBRS_ERR_INVALID, "the HMM handle is on device %d, the scan on device %d", view.device, s->device);
    if (view.H != s->H) return fail(GBRS_ERR_INVALID, "the HMM handle has %d founders, the scan %d", view.H, s->H);
    if ((int)view.points.size() != s->n_chrom)
        return fail(GBRS_ERR_INVALID, "the HMM handle has %d chromosomes, the scan %d", (int)view.points.size(), s->n_chrom);
    for (int c = 0; c < s->n_chrom; ++c)
        if (view.points[c] != s->points[c])
            return fail(GBRS_ERR_INVALID, "grid mismatch: chromosome %d has %d grid points on the HMM handle, %d on the scan", c,
                        view.points[c], s->points[c]);
    if (s->cohort.n + view.n > std::numeric_limits<int32_t>::max() / 16) return fail(GBRS_ERR_INVALID, "too many samples");
    GBRS_TRY(hmm_grid_view(hmm, sample, &view, true));
    GBRS_TRY(scan_reserve(s, view.n));
    const size_t row = (size_t)s->M * s->H;
    GBRS_HIP_CHECK(hipMemcpyAsync(s->cohort.dosage.p + (size_t)s->cohort.n * row, view.dosage, (size_t)view.n * row * sizeof(double),
                                  hipMemcpyDeviceToDevice, s->stream));
    GBRS_HIP_CHECK(hipStreamSynchronize(s->stream));
    scan_appended(s, view.n);
    return GBRS_OK;
}

int gbrs_scan_prepare(gbrs_scan_t *s, int c, const double *qz) {
    RoctxRange roctx_range("gbrs_scan_prepare");
    if (!s) return fail(GBRS_ERR_INVALID, "handle is NULL");
    if (c < 1 || c > SC_MAX_C) return fail(GBRS_ERR_INVALID, "covariate columns must be 1..%d (the intercept included), got %d", SC_MAX_C, c);
    if (!qz) return fail(GBRS_ERR_INVALID, "qz is NULL");
    if (s->cohort.n <= (int64_t)c + s->H - 1)
        return fail(GBRS_ERR_INVALID, "%lld samples are too few for %d covariate columns and %d founders: need more than %d",
                    (long long)s->cohort.n, c, s->H, c + s->H - 1);
    const int n = (int)s->cohort.n;
    for (int64_t k = 0; k < (int64_t)n * c; ++k)
        if (!std::isfinite(qz[k]))
            return fail(GBRS_ERR_INVALID, "covariate basis holds a value that is not finite (sample %lld, column %d)", (long long)(k / c),
                        (int)(k % c));
    GBRS_TRY(select_device(s->device));
    gbrs_scan::Prep &pr = s->prep;
    pr.unprepare();                     // the arguments are good: from here on W is being overwritten
    const int64_t n_ld = padded(n);
    const size_t n_w = (size_t)s->M * s->Hp * n_ld;
    if (pr.qz.n != (size_t)n * c) GBRS_TRY(pr.qz.alloc((size_t)n * c));
    if (pr.W.n != n_w) GBRS_TRY(pr.W.alloc(n_w));
    if (pr.d_rank.n != (size_t)s->M) GBRS_TRY(pr.d_rank.alloc((size_t)s->M));
    GBRS_HIP_CHECK(hipMemcpy(pr.qz.p, qz, pr.qz.bytes(), hipMemcpyHostToDevice));
    GBRS_TRY(timed_open(s));
    auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3((unsigned)s->M), dim3(SC_THREADS), 0, s->stream, n, s->M, s->H, c, n_ld, s->cohort.dosage.p, pr.qz.p,
                           pr.W.p, pr.d_rank.p);
    };
    if (s->Hp == 8) launch(scan_prepare_kernel<8>);
    else launch(scan_prepare_kernel<16>);
    GBRS_TRY(timed_wait(s));
    s->last.scan.last_prepare_ms = pass_ms(s, s->last.scan.last_prepare_ms);
    std::vector<int32_t> rank((size_t)s->M);
    GBRS_TRY(copy_out(rank.data(), pr.d_rank, pr.d_rank.n));
    pr.rank.swap(rank);
    pr.n_ld = n_ld;
    pr.c = c;
    return GBRS_OK;
}

}  // extern "C"

namespace {

// a buffer of the handle's chunk that follows the last call's size
template <typename T>
int resized(DevBuf<T> &buf, size_t n) { return buf.n != n ? buf.alloc(n) : GBRS_OK; }

// The pass of gbrs_scan_run.  With support, gbrs_scan_run_support's: the intervals of every chunk follow its peaks while
// its LOD rows are on the device; the two tables of a chunk are the call's own, so the handle holds what it held.
int scan_run_pass(gbrs_scan *s, int64_t P, const double *pheno, bool support, double drop, double *lod, double *peak_lod,
                  int64_t *peak_index, int64_t *support_lo, int64_t *support_hi) {
    if (!s) return fail(GBRS_ERR_INVALID, "handle is NULL");
    if (s->prep.c == 0) return fail(GBRS_ERR_INVALID, "no covariates on the handle: call gbrs_scan_prepare first");
    if (P < 1 || !pheno) return fail(GBRS_ERR_INVALID, "bad argument");
    if (support && !(drop >= 0.0 && std::isfinite(drop)))
        return fail(GBRS_ERR_INVALID, "the LOD drop of a support interval must be a finite number that is not negative, got %g", drop);
    const int n = (int)s->cohort.n, nc = s->n_chrom;
    GBRS_TRY(check_finite("phenotype", pheno, n, P));
    GBRS_TRY(select_device(s->device));
    gbrs_scan::Prep &pr = s->prep;
    const int64_t pc_max = std::min(P, SC_PCHUNK), M = s->M, n_ld = pr.n_ld;
    GBRS_TRY(resized(pr.y, (size_t)n * pc_max));
    GBRS_TRY(resized(pr.yt, (size_t)pc_max * n_ld));
    GBRS_TRY(resized(pr.rss0, (size_t)pc_max));
    GBRS_TRY(resized(pr.lod, (size_t)pc_max * M));
    GBRS_TRY(resized(pr.peak_lod, (size_t)pc_max * nc));
    GBRS_TRY(resized(pr.peak_index, (size_t)pc_max * nc));
    DevBuf<int64_t> d_lo, d_hi;
    if (support) {
        GBRS_TRY(d_lo.alloc((size_t)pc_max * nc));
        GBRS_TRY(d_hi.alloc((size_t)pc_max * nc));
    }
    const unsigned row_blocks = (unsigned)((M * s->Hp + SC_ROWS - 1) / SC_ROWS);
    double t_product = 0.0;
    GBRS_TRY(timed_open(s));
    for (int64_t p0 = 0; p0 < P; p0 += SC_PCHUNK) {
        const int64_t pc = std::min(SC_PCHUNK, P - p0);
        const size_t peaks = (size_t)pc * nc;
        GBRS_TRY(project(s, pr.qz, pr.c, n_ld, pheno, P, p0, pc, pr.y, pr.yt.p, pr.rss0.p));
        GBRS_HIP_CHECK(hipEventRecord(s->ev[2], s->stream));
        const dim3 grid(row_blocks, (unsigned)((pc + SC_COLS - 1) / SC_COLS));
        auto launch = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, grid, dim3(SC_THREADS), 0, s->stream, M, pc, n_ld, 0.5 * n, pr.W.p, pr.yt.p, pr.rss0.p, pr.lod.p);
        };
        if (s->Hp == 8) launch(scan_lod_kernel<8>);
        else launch(scan_lod_kernel<16>);
        GBRS_HIP_CHECK(hipEventRecord(s->ev[3], s->stream));
        hipLaunchKernelGGL(scan_peak_kernel, dim3((unsigned)nc, (unsigned)pc), dim3(64), 0, s->stream, M, nc, s->d_point_off.p, pr.lod.p,
                           pr.peak_lod.p, pr.peak_index.p);
        if (support)
            hipLaunchKernelGGL(scan_support_kernel, dim3((unsigned)nc, (unsigned)pc), dim3(64), 0, s->stream, M, nc, drop,
                               s->d_point_off.p, pr.lod.p, pr.peak_lod.p, pr.peak_index.p, d_lo.p, d_hi.p);
        GBRS_HIP_CHECK(hipGetLastError());
        GBRS_HIP_CHECK(hipStreamSynchronize(s->stream));
        t_product += elapsed_ms(s->ev[2], s->ev[3], 0.0);
        GBRS_TRY(copy_out(lod, pr.lod, (size_t)pc * M, (size_t)p0 * M));
        GBRS_TRY(copy_out(peak_lod, pr.peak_lod, peaks, (size_t)p0 * nc));
        GBRS_TRY(copy_out(peak_index, pr.peak_index, peaks, (size_t)p0 * nc));
        GBRS_TRY(copy_out(support_lo, d_lo, peaks, (size_t)p0 * nc));
        GBRS_TRY(copy_out(support_hi, d_hi, peaks, (size_t)p0 * nc));
    }
    GBRS_TRY(timed_wait(s));
    s->last.scan.last_run_ms = pass_ms(s, s->last.scan.last_run_ms);
    s->last.scan.last_product_ms = t_product;
    return GBRS_OK;
}

}  // namespace

extern "C" {

int gbrs_scan_run(gbrs_scan_t *s, int64_t P, const double *pheno, double *lod, double *peak_lod, int64_t *peak_index) {
    RoctxRange roctx_range("gbrs_scan_run");
    return scan_run_pass(s, P, pheno, false, 0.0, lod, peak_lod, peak_index, nullptr, nullptr);
}

int gbrs_scan_run_support(gbrs_scan_t *s, int64_t P, const double *pheno, double drop, double *lod, double *peak_lod,
                          int64_t *peak_index, int64_t *support_lo, int64_t *support_hi) {
    RoctxRange roctx_range("gbrs_scan_run_support");
    return scan_run_pass(s, P, pheno, true, drop, lod, peak_lod, peak_index, support_lo, support_hi);
}

int gbrs_scan_permute(gbrs_scan_t *s, int64_t P, const double *pheno, int64_t B, uint64_t seed, const uint8_t *chrom_mask,
                      double *perm_max, int32_t *perm_index) {
    RoctxRange roctx_range("gbrs_scan_permute");
    if (!s) return fail(GBRS_ERR_INVALID, "handle is NULL");
    if (s->prep.c == 0) return fail(GBRS_ERR_INVALID, "no covariates on the handle: call gbrs_scan_prepare first");
    if (P < 1) return fail(GBRS_ERR_INVALID, "a permutation pass needs at least 1 phenotype, got %lld", (long long)P);
    if (B < 1) return fail(GBRS_ERR_INVALID, "a permutation pass needs at least 1 permutation, got %lld", (long long)B);
    if (!pheno || !perm_max) return fail(GBRS_ERR_INVALID, "bad argument");
    const int n = (int)s->cohort.n, nc = s->n_chrom;
    const int tiles = (n + SP_THREADS - 1) / SP_THREADS;
    if (B > std::numeric_limits<int32_t>::max() / tiles || P > std::numeric_limits<int64_t>::max() / 8 / B)
        return fail(GBRS_ERR_INVALID, "too many permutations: %lld of %d samples for %lld phenotypes", (long long)B, n, (long long)P);
    int64_t selected = 0;
    for (int c = 0; c < nc; ++c)
        if (!chrom_mask || chrom_mask[c]) selected += s->points[c];
    if (selected == 0) return fail(GBRS_ERR_INVALID, "the chromosome mask selects no grid point");
    GBRS_TRY(check_finite("phenotype", pheno, n, P));
    GBRS_TRY(select_device(s->device));
    const gbrs_scan::Prep &pr = s->prep;
    const int64_t cols = P * B, pc_max = std::min(cols, SC_PCHUNK), yc_max = std::min(P, SC_PCHUNK), M = s->M, n_ld = pr.n_ld;
    Tally own;
    DevBuf<double> y, yt_all, rss_all, yt, rss0, lod, peak_lod, pmax;
    DevBuf<int64_t> peak_index;
    DevBuf<int32_t> perm;
    DevBuf<uint8_t> mask;
    GBRS_TRY(own.alloc(y, (size_t)n * yc_max));
    GBRS_TRY(own.alloc(yt_all, (size_t)P * n_ld));
    GBRS_TRY(own.alloc(rss_all, (size_t)P));
    GBRS_TRY(own.alloc(yt, (size_t)pc_max * n_ld));
    GBRS_TRY(own.alloc(rss0, (size_t)pc_max));
    GBRS_TRY(own.alloc(lod, (size_t)pc_max * M));
    GBRS_TRY(own.alloc(peak_lod, (size_t)pc_max * nc));
    GBRS_TRY(own.alloc(peak_index, (size_t)pc_max * nc));
    GBRS_TRY(own.alloc(pmax, (size_t)cols));
    GBRS_TRY(own.alloc(perm, (size_t)B * n));
    GBRS_TRY(own.alloc(mask, (size_t)nc));
    std::vector<uint8_t> h_mask((size_t)nc, 1);
    if (chrom_mask)
        for (int c = 0; c < nc; ++c) h_mask[c] = chrom_mask[c] ? 1 : 0;
    GBRS_HIP_CHECK(hipMemcpy(mask.p, h_mask.data(), mask.bytes(), hipMemcpyHostToDevice));
    EventRing ring;
    GBRS_TRY(ring.create());
    GBRS_TRY(timed_open(s));
    GBRS_TRY(project_all(s, pr.qz, pr.c, n_ld, pheno, P, y, yt_all, rss_all));
    hipLaunchKernelGGL(scan_perm_rank_kernel, dim3((unsigned)(B * tiles)), dim3(SP_THREADS), 0, s->stream, n, tiles,
                       (uint32_t)(seed & 0xFFFFFFFFu), (uint32_t)(seed >> 32), perm.p);
    GBRS_HIP_CHECK(hipGetLastError());
    const unsigned row_blocks = (unsigned)((M * s->Hp + SC_ROWS - 1) / SC_ROWS);
    for (int64_t col0 = 0; col0 < cols; col0 += SC_PCHUNK) {
        const int64_t pc = std::min(SC_PCHUNK, cols - col0);
        int slot = 0;
        GBRS_TRY(ring.next(&slot));
        hipLaunchKernelGGL(scan_perm_pheno_kernel, dim3((unsigned)pc), dim3(64), 0, s->stream, n, pr.c, n_ld, B, col0, yt_all.p,
                           perm.p, pr.qz.p, yt.p, rss0.p);
        GBRS_HIP_CHECK(hipEventRecord(ring.ev[2 * slot], s->stream));
        const dim3 grid(row_blocks, (unsigned)((pc + SC_COLS - 1) / SC_COLS));
        auto launch = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, grid, dim3(SC_THREADS), 0, s->stream, M, pc, n_ld, 0.5 * n, pr.W.p, yt.p, rss0.p, lod.p);
        };
        if (s->Hp == 8) launch(scan_lod_kernel<8>);
        else launch(scan_lod_kernel<16>);
        GBRS_HIP_CHECK(hipEventRecord(ring.ev[2 * slot + 1], s->stream));
        hipLaunchKernelGGL(scan_peak_kernel, dim3((unsigned)nc, (unsigned)pc), dim3(64), 0, s->stream, M, nc, s->d_point_off.p, lod.p,
                           peak_lod.p, peak_index.p);
        hipLaunchKernelGGL(scan_perm_max_kernel, dim3((unsigned)((pc + SP_THREADS - 1) / SP_THREADS)), dim3(SP_THREADS), 0, s->stream,
                           pc, nc, s->d_point_off.p, mask.p, peak_lod.p, pmax.p + col0);
        GBRS_HIP_CHECK(hipGetLastError());
    }
    GBRS_TRY(timed_wait(s));
    GBRS_TRY(ring.drain());
    GBRS_TRY(copy_out(perm_max, pmax, pmax.n));
    GBRS_TRY(copy_out(perm_index, perm, perm.n));
    gbrs_scan_perm_info_t &r = s->last.perm;
    r.P = P;
    r.B = B;
    r.last_permute_ms = pass_ms(s, r.last_permute_ms);
    r.last_product_ms = ring.ms;
    r.peak_device_bytes = s->resident_bytes() + own.bytes;
    return GBRS_OK;
}

int gbrs_scan_perm_info(gbrs_scan_t *s, gbrs_scan_perm_info_t *info) {
    if (!s || !info) return fail(GBRS_ERR_INVALID, "bad argument");
    *info = s->last.perm;
    return GBRS_OK;
}

int gbrs_scan_set_snps(gbrs_scan_t *s, const double *const *grid_pos, const int64_t *n_snps, const double *const *snp_pos,
                       const uint32_t *const *snp_mask) {
    RoctxRange roctx_range("gbrs_scan_set_snps");
    if (!s) return fail(GBRS_ERR_INVALID, "handle is NULL");
    if (!n_snps) return fail(GBRS_ERR_INVALID, "n_snps is NULL");
    std::vector<int64_t> off((size_t)s->n_chrom + 1, 0);
    for (int c = 0; c < s->n_chrom; ++c) {
        if (n_snps[c] < 0) return fail(GBRS_ERR_INVALID, "chromosome %d has a negative number of SNPs", c);
        off[c + 1] = off[c] + n_snps[c];
    }
    const int64_t M_snp = off[s->n_chrom];
    if (M_snp == 0) {                   // all-zero counts drop the SNPs
        s->snp.clear();
        return GBRS_OK;
    }
    if (!grid_pos || !snp_pos || !snp_mask) return fail(GBRS_ERR_INVALID, "bad argument");
    const uint32_t beyond = s->H >= 32 ? 0u : ~0u << s->H;
    for (int c = 0; c < s->n_chrom; ++c) {
        const int64_t k = s->points[c];
        if (k > 0 && !grid_pos[c]) return fail(GBRS_ERR_INVALID, "chromosome %d has no grid positions", c);
        for (int64_t i = 0; i < k; ++i) {
            if (!std::isfinite(grid_pos[c][i]))
                return fail(GBRS_ERR_INVALID, "grid position %lld of chromosome %d is not finite", (long long)i, c);
            if (i > 0 && grid_pos[c][i] < grid_pos[c][i - 1])
                return fail(GBRS_ERR_INVALID, "the grid positions of chromosome %d decrease at index %lld", c, (long long)i);
        }
        if (n_snps[c] == 0) continue;
        if (k == 0) return fail(GBRS_ERR_INVALID, "chromosome %d has %lld SNPs and no grid point", c, (long long)n_snps[c]);
        if (!snp_pos[c] || !snp_mask[c]) return fail(GBRS_ERR_INVALID, "chromosome %d has SNPs and no positions or patterns", c);
        for (int64_t i = 0; i < n_snps[c]; ++i) {
            if (!std::isfinite(snp_pos[c][i]))
                return fail(GBRS_ERR_INVALID, "SNP %lld of chromosome %d has a position that is not finite", (long long)i, c);
            if (snp_mask[c][i] & beyond)
                return fail(GBRS_ERR_INVALID, "SNP %lld of chromosome %d has a pattern bit at or above the %d founders", (long long)i, c,
                            s->H);
        }
    }
    GBRS_TRY(select_device(s->device));
    // everything is built beside what the handle holds and swapped in at the end: a failure leaves the handle as it was
    std::vector<double> h_grid((size_t)s->M), h_pos((size_t)M_snp);
    std::vector<uint32_t> h_mask((size_t)M_snp);
    for (int c = 0; c < s->n_chrom; ++c) {
        if (s->points[c] > 0) std::memcpy(h_grid.data() + s->point_off[c], grid_pos[c], (size_t)s->points[c] * sizeof(double));
        if (n_snps[c] > 0) {
            std::memcpy(h_pos.data() + off[c], snp_pos[c], (size_t)n_snps[c] * sizeof(double));
            std::memcpy(h_mask.data() + off[c], snp_mask[c], (size_t)n_snps[c] * sizeof(uint32_t));
        }
    }
    DevBuf<double> d_grid, d_pos, d_t;
    DevBuf<int64_t> d_off;
    DevBuf<int32_t> d_lo, d_hi;
    DevBuf<uint32_t> d_mask;
    GBRS_TRY(d_grid.alloc(h_grid.size()));
    GBRS_TRY(d_pos.alloc(h_pos.size()));
    GBRS_TRY(d_t.alloc((size_t)M_snp));
    GBRS_TRY(d_off.alloc(off.size()));
    GBRS_TRY(d_lo.alloc((size_t)M_snp));
    GBRS_TRY(d_hi.alloc((size_t)M_snp));
    GBRS_TRY(d_mask.alloc((size_t)M_snp));
    GBRS_HIP_CHECK(hipMemcpy(d_grid.p, h_grid.data(), d_grid.bytes(), hipMemcpyHostToDevice));
    GBRS_HIP_CHECK(hipMemcpy(d_pos.p, h_pos.data(), d_pos.bytes(), hipMemcpyHostToDevice));
    GBRS_HIP_CHECK(hipMemcpy(d_mask.p, h_mask.data(), d_mask.bytes(), hipMemcpyHostToDevice));
    GBRS_HIP_CHECK(hipMemcpy(d_off.p, off.data(), d_off.bytes(), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(scan_snp_locate_kernel, dim3((unsigned)((M_snp + SC_THREADS - 1) / SC_THREADS)), dim3(SC_THREADS), 0, s->stream,
                       M_snp, s->n_chrom, d_off.p, s->d_point_off.p, d_grid.p, d_pos.p, d_lo.p, d_hi.p, d_t.p);
    GBRS_HIP_CHECK(hipGetLastError());
    GBRS_HIP_CHECK(hipStreamSynchronize(s->stream));
    s->snp.d_off.swap(d_off);
    s->snp.lo.swap(d_lo);
    s->snp.hi.swap(d_hi);
    s->snp.mask.swap(d_mask);
    s->snp.t.swap(d_t);
    s->snp.off.swap(off);
    s->snp.M = M_snp;
    return GBRS_OK;
}

int gbrs_scan_snp_dosage(gbrs_scan_t *s, int64_t first, int64_t count, double *out) {
    RoctxRange roctx_range("gbrs_scan_snp_dosage");
    if (!s) return fail(GBRS_ERR_INVALID, "handle is NULL");
    if (s->snp.M == 0) return fail(GBRS_ERR_INVALID, "no SNPs on the handle: call gbrs_scan_set_snps first");
    if (s->cohort.n == 0) return fail(GBRS_ERR_INVALID, "no samples on the handle");
    if (first < 0 || count < 0 || first > s->snp.M || count > s->snp.M - first)
        return fail(GBRS_ERR_INVALID, "SNPs %lld .. %lld are out of range: the handle has %lld", (long long)first,
                    (long long)(first + count), (long long)s->snp.M);
    if (count == 0) return GBRS_OK;
    if (!out) return fail(GBRS_ERR_INVALID, "out is NULL");
    GBRS_TRY(select_device(s->device));
    const int n = (int)s->cohort.n;
    const int64_t step = std::max<int64_t>(1, std::min(count, ((int64_t)1 << 24) / n));     // at most 128 MB of workspace
    DevBuf<double> buf;
    GBRS_TRY(buf.alloc((size_t)n * step));
    for (int64_t j0 = 0; j0 < count; j0 += step) {
        const int64_t jc = std::min(step, count - j0);
        hipLaunchKernelGGL(scan_snp_dosage_kernel, dim3((unsigned)((n * jc + SC_THREADS - 1) / SC_THREADS)), dim3(SC_THREADS), 0,
                           s->stream, n, s->M, s->H, first + j0, jc, s->cohort.dosage.p, s->snp.lo.p, s->snp.hi.p, s->snp.mask.p,
                           s->snp.t.p, buf.p);
        GBRS_HIP_CHECK(hipGetLastError());
        GBRS_HIP_CHECK(hipMemcpy2DAsync(out + j0, (size_t)count * sizeof(double), buf.p, (size_t)jc * sizeof(double),
                                        (size_t)jc * sizeof(double), (size_t)n, hipMemcpyDeviceToHost, s->stream));
        GBRS_HIP_CHECK(hipStreamSynchronize(s->stream));
    }
    return GBRS_OK;
}

int gbrs_scan_snps(gbrs_scan_t *s, int64_t P, const double *pheno, double *lod, uint8_t *used, double *peak_lod,
                   int64_t *peak_index) {
    RoctxRange roctx_range("gbrs_scan_snps");
    if (!s) return fail(GBRS_ERR_INVALID, "handle is NULL");
    if (s->prep.c == 0) return fail(GBRS_ERR_INVALID, "no covariates on the handle: call gbrs_scan_prepare first");
    if (s->snp.M == 0) return fail(GBRS_ERR_INVALID, "no SNPs on the handle: call gbrs_scan_set_snps first");
    if (P < 1) return fail(GBRS_ERR_INVALID, "a SNP pass needs at least 1 phenotype, got %lld", (long long)P);
    if (!pheno) return fail(GBRS_ERR_INVALID, "bad argument");
    const int n = (int)s->cohort.n;
    GBRS_TRY(check_finite("phenotype", pheno, n, P));
    GBRS_TRY(select_device(s->device));
    const gbrs_scan::Prep &pr = s->prep;
    const gbrs_scan::Snp &sn = s->snp;
    const int64_t M_snp = sn.M, n_ld = pr.n_ld, yc_max = std::min(P, SC_PCHUNK), lc_max = std::min(M_snp, SS_CHUNK);
    const int nc = s->n_chrom;
    // the two points of a run in LDS when the device has the room
    int lds_max = 0;
    GBRS_HIP_CHECK(hipDeviceGetAttribute(&lds_max, hipDeviceAttributeMaxSharedMemoryPerBlock, s->device));
    const size_t pair_bytes = (size_t)2 * s->H * (n | 1) * sizeof(double);
    const int staged = pair_bytes <= (size_t)lds_max;
    if (staged)
        GBRS_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(scan_snp_row_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                           (int)pair_bytes));
    Tally own;
    DevBuf<double> y, yt_all, rss_all, w, d_lod, d_peak;
    DevBuf<int64_t> d_index;
    DevBuf<uint8_t> d_used;
    GBRS_TRY(own.alloc(y, (size_t)n * yc_max));
    GBRS_TRY(own.alloc(yt_all, (size_t)P * n_ld));
    GBRS_TRY(own.alloc(rss_all, (size_t)P));
    GBRS_TRY(own.alloc(w, (size_t)lc_max * n_ld));
    GBRS_TRY(own.alloc(d_lod, (size_t)yc_max * lc_max));
    GBRS_TRY(own.alloc(d_used, (size_t)lc_max));
    GBRS_TRY(own.alloc(d_peak, (size_t)P * nc));
    GBRS_TRY(own.alloc(d_index, (size_t)P * nc));
    EventRing row_ring, product_ring;
    GBRS_TRY(row_ring.create());
    GBRS_TRY(product_ring.create());
    GBRS_TRY(timed_open(s));
    GBRS_HIP_CHECK(hipMemsetAsync(d_index.p, 0xFF, d_index.bytes(), s->stream));         // -1: nothing yet
    GBRS_TRY(project_all(s, pr.qz, pr.c, n_ld, pheno, P, y, yt_all, rss_all));
    for (int64_t j0 = 0; j0 < M_snp; j0 += SS_CHUNK) {
        const int64_t jc = std::min(SS_CHUNK, M_snp - j0);
        int slot = 0;
        GBRS_TRY(row_ring.next(&slot));
        GBRS_HIP_CHECK(hipEventRecord(row_ring.ev[2 * slot], s->stream));
        hipLaunchKernelGGL(scan_snp_row_kernel, dim3((unsigned)((jc + SS_BLOCK - 1) / SS_BLOCK)), dim3(SC_THREADS),
                           staged ? pair_bytes : 0, s->stream, n, s->M, s->H, pr.c, n_ld, j0, jc, staged, s->cohort.dosage.p, pr.qz.p,
                           sn.lo.p, sn.hi.p, sn.mask.p, sn.t.p, w.p, d_used.p);
        GBRS_HIP_CHECK(hipEventRecord(row_ring.ev[2 * slot + 1], s->stream));
        GBRS_HIP_CHECK(hipGetLastError());
        if (used) GBRS_HIP_CHECK(hipMemcpyAsync(used + j0, d_used.p, (size_t)jc, hipMemcpyDeviceToHost, s->stream));
        for (int64_t p0 = 0; p0 < P; p0 += SC_PCHUNK) {
            const int64_t pc = std::min(SC_PCHUNK, P - p0);
            GBRS_TRY(product_ring.next(&slot));
            GBRS_HIP_CHECK(hipEventRecord(product_ring.ev[2 * slot], s->stream));
            hipLaunchKernelGGL(scan_snp_lod_kernel, dim3((unsigned)((jc + SC_ROWS - 1) / SC_ROWS), (unsigned)((pc + SC_COLS - 1) / SC_COLS)),
                               dim3(SC_THREADS), 0, s->stream, jc, pc, n_ld, jc, 0.5 * n, w.p, yt_all.p + p0 * n_ld, rss_all.p + p0,
                               d_lod.p);
            GBRS_HIP_CHECK(hipEventRecord(product_ring.ev[2 * slot + 1], s->stream));
            hipLaunchKernelGGL(scan_snp_peak_kernel, dim3((unsigned)nc, (unsigned)pc), dim3(64), 0, s->stream, j0, jc, jc, nc,
                               sn.d_off.p, d_used.p, d_lod.p, d_peak.p + p0 * nc, d_index.p + p0 * nc);
            GBRS_HIP_CHECK(hipGetLastError());
            if (lod)        // waits for the kernels before it on the stream; the next chunk's product overwrites d_lod after it
                GBRS_HIP_CHECK(hipMemcpy2DAsync(lod + p0 * M_snp + j0, (size_t)M_snp * sizeof(double), d_lod.p,
                                                (size_t)jc * sizeof(double), (size_t)jc * sizeof(double), (size_t)pc,
                                                hipMemcpyDeviceToHost, s->stream));
        }
    }
    GBRS_TRY(timed_wait(s));
    GBRS_TRY(row_ring.drain());
    GBRS_TRY(product_ring.drain());
    GBRS_TRY(snp_peaks_out(d_peak, d_index, peak_lod, peak_index));
    gbrs_scan_snp_info_t &r = s->last.snp;
    r.P = P;
    r.staged = staged;
    r.last_pass_ms = pass_ms(s, r.last_pass_ms);
    r.last_row_ms = row_ring.ms;
    r.last_product_ms = product_ring.ms;
    r.peak_device_bytes = s->resident_bytes() + own.bytes;
    return GBRS_OK;
}

int gbrs_scan_snp_info(gbrs_scan_t *s, gbrs_scan_snp_info_t *info) {
    if (!s || !info) return fail(GBRS_ERR_INVALID, "bad argument");
    *info = s->last.snp;
    info->M_snp = s->snp.M;
    info->chunk = SS_CHUNK;
    info->device_bytes = s->snp.bytes();
    return GBRS_OK;
}

int gbrs_scan_mediate(gbrs_scan_t *s, int64_t T, const double *target, const int64_t *point, int64_t Q, const double *mediator,
                      int K, double *lod0, double *lod_med, uint8_t *used, double *best_lod, int64_t *best_index, double *mean,
                      double *sd, int64_t *n_used) {
    RoctxRange roctx_range("gbrs_scan_mediate");
    if (!s) return fail(GBRS_ERR_INVALID, "handle is NULL");
    if (s->prep.c == 0) return fail(GBRS_ERR_INVALID, "no covariates on the handle: call gbrs_scan_prepare first");
    if (T < 1) return fail(GBRS_ERR_INVALID, "a mediation pass needs at least 1 target, got %lld", (long long)T);
    if (Q < 1) return fail(GBRS_ERR_INVALID, "a mediation pass needs at least 1 mediator, got %lld", (long long)Q);
    if (K < 0 || K > SM_MAX_K) return fail(GBRS_ERR_INVALID, "the top list has 0..%d places, got %d", SM_MAX_K, K);
    if (!target || !point || !mediator || (K > 0 && (!best_lod || !best_index))) return fail(GBRS_ERR_INVALID, "bad argument");
    const gbrs_scan::Prep &pr = s->prep;
    if (s->cohort.n <= (int64_t)pr.c + s->H)
        return fail(GBRS_ERR_INVALID, "%lld samples are too few to mediate with %d covariate columns and %d founders: the mediator "
                    "takes one more degree of freedom, need more than %d", (long long)s->cohort.n, pr.c, s->H, pr.c + s->H);
    if (Q > std::numeric_limits<int64_t>::max() / 16 / std::min(T, SM_TCHUNK) || (Q + SC_COLS - 1) / SC_COLS > std::numeric_limits<int32_t>::max())
        return fail(GBRS_ERR_INVALID, "too many mediators: %lld", (long long)Q);
    GBRS_TRY(check_targets(s, T, nullptr, 0, point));
    const int n = (int)s->cohort.n;
    GBRS_TRY(check_finite("target", target, n, T));
    GBRS_TRY(check_finite("mediator", mediator, n, Q));
    GBRS_TRY(select_device(s->device));
    const int64_t n_ld = pr.n_ld, tc_max = std::min(T, SM_TCHUNK), yc_max = std::max(std::min(Q, SC_PCHUNK), tc_max);
    const int Hp = s->Hp, pts = SC_ROWS / Hp;
    Tally own;
    DevBuf<double> y, zt, szz, yt, syy, a, rss1, d_lod0, d_lod, d_best, d_mean, d_sd;
    DevBuf<int64_t> d_point, d_index, d_count;
    DevBuf<uint8_t> d_used;
    GBRS_TRY(own.alloc(y, (size_t)n * yc_max));
    GBRS_TRY(own.alloc(zt, (size_t)Q * n_ld));
    GBRS_TRY(own.alloc(szz, (size_t)Q));
    GBRS_TRY(own.alloc(yt, (size_t)tc_max * n_ld));
    GBRS_TRY(own.alloc(syy, (size_t)tc_max));
    GBRS_TRY(own.alloc(a, (size_t)tc_max * Hp));
    GBRS_TRY(own.alloc(rss1, (size_t)tc_max));
    GBRS_TRY(own.alloc(d_lod0, (size_t)T));
    GBRS_TRY(own.alloc(d_lod, (size_t)tc_max * Q));
    GBRS_TRY(own.alloc(d_used, (size_t)tc_max * Q));
    GBRS_TRY(own.alloc(d_best, (size_t)T * K));
    GBRS_TRY(own.alloc(d_index, (size_t)T * K));
    GBRS_TRY(own.alloc(d_mean, (size_t)T));
    GBRS_TRY(own.alloc(d_sd, (size_t)T));
    GBRS_TRY(own.alloc(d_count, (size_t)T));
    GBRS_TRY(own.alloc(d_point, (size_t)T));
    GBRS_HIP_CHECK(hipMemcpy(d_point.p, point, d_point.bytes(), hipMemcpyHostToDevice));
    EventRing ring;
    GBRS_TRY(ring.create());
    GBRS_TRY(timed_open(s));
    GBRS_TRY(project_all(s, pr.qz, pr.c, n_ld, mediator, Q, y, zt, szz));            // z~ of every mediator
    for (int64_t t0 = 0; t0 < T; t0 += SM_TCHUNK) {
        const int64_t tc = std::min(SM_TCHUNK, T - t0);
        GBRS_TRY(project(s, pr.qz, pr.c, n_ld, target, T, t0, tc, y, yt.p, syy.p));
        auto targets = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, dim3((unsigned)tc), dim3(64), 0, s->stream, n_ld, 0.5 * n, pr.W.p, d_point.p + t0, yt.p, syy.p,
                               a.p, rss1.p, d_lod0.p + t0);
        };
        if (Hp == 8) targets(scan_med_target_kernel<8>);
        else targets(scan_med_target_kernel<16>);
        int slot = 0;
        GBRS_TRY(ring.next(&slot));
        GBRS_HIP_CHECK(hipEventRecord(ring.ev[2 * slot], s->stream));
        const dim3 grid((unsigned)((Q + SC_COLS - 1) / SC_COLS), (unsigned)((tc + pts - 1) / pts));
        auto product = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, grid, dim3(SC_THREADS), 0, s->stream, tc, Q, n_ld, 0.5 * n, pr.W.p, d_point.p + t0, yt.p, zt.p,
                               syy.p, rss1.p, a.p, szz.p, d_lod.p, d_used.p);
        };
        if (Hp == 8) product(scan_med_kernel<8>);
        else product(scan_med_kernel<16>);
        GBRS_HIP_CHECK(hipEventRecord(ring.ev[2 * slot + 1], s->stream));
        hipLaunchKernelGGL(scan_med_select_kernel, dim3((unsigned)tc), dim3(64), 0, s->stream, Q, K, d_lod.p, d_used.p,
                           d_best.p + t0 * K, d_index.p + t0 * K, d_mean.p + t0, d_sd.p + t0, d_count.p + t0);
        GBRS_HIP_CHECK(hipGetLastError());
        // the copies wait for the kernels before them on the stream; the next chunk's product overwrites d_lod after them
        if (lod_med)
            GBRS_HIP_CHECK(hipMemcpyAsync(lod_med + t0 * Q, d_lod.p, (size_t)tc * Q * sizeof(double), hipMemcpyDeviceToHost, s->stream));
        if (used) GBRS_HIP_CHECK(hipMemcpyAsync(used + t0 * Q, d_used.p, (size_t)tc * Q, hipMemcpyDeviceToHost, s->stream));
    }
    GBRS_TRY(timed_wait(s));
    GBRS_TRY(ring.drain());
    GBRS_TRY(copy_out(lod0, d_lod0, d_lod0.n));
    if (K > 0) {
        GBRS_TRY(copy_out(best_lod, d_best, d_best.n));
        GBRS_TRY(copy_out(best_index, d_index, d_index.n));
    }
    GBRS_TRY(copy_out(mean, d_mean, d_mean.n));
    GBRS_TRY(copy_out(sd, d_sd, d_sd.n));
    GBRS_TRY(copy_out(n_used, d_count, d_count.n));
    gbrs_scan_mediate_info_t &r = s->last.mediate;
    r.T = T;
    r.Q = Q;
    r.last_pass_ms = pass_ms(s, r.last_pass_ms);
    r.last_product_ms = ring.ms;
    r.peak_device_bytes = s->resident_bytes() + own.bytes;
    return GBRS_OK;
}

int gbrs_scan_mediate_info(gbrs_scan_t *s, gbrs_scan_mediate_info_t *info) {
    if (!s || !info) return fail(GBRS_ERR_INVALID, "bad argument");
    *info = s->last.mediate;
    return GBRS_OK;
}

int gbrs_scan_effects(gbrs_scan_t *s, int64_t P, const double *pheno, int64_t T, const int64_t *column, const int64_t *point,
                      double *effect, double *se, double *lod, double *sigma2, int32_t *rank) {
    RoctxRange roctx_range("gbrs_scan_effects");
    if (!s) return fail(GBRS_ERR_INVALID, "handle is NULL");
    if (s->prep.c == 0) return fail(GBRS_ERR_INVALID, "no covariates on the handle: call gbrs_scan_prepare first");
    if (P < 1) return fail(GBRS_ERR_INVALID, "an effects pass needs at least 1 phenotype, got %lld", (long long)P);
    if (T < 1) return fail(GBRS_ERR_INVALID, "an effects pass needs at least 1 target, got %lld", (long long)T);
    if (!pheno || !column || !point) return fail(GBRS_ERR_INVALID, "bad argument");
    GBRS_TRY(check_targets(s, T, column, P, point));
    const int n = (int)s->cohort.n;
    GBRS_TRY(check_finite("phenotype", pheno, n, P));
    GBRS_TRY(select_device(s->device));
    const gbrs_scan::Prep &pr = s->prep;
    const int64_t n_ld = pr.n_ld, tc_max = std::min(T, SE_TCHUNK), yc_max = std::min(P, SC_PCHUNK);
    const int H = s->H, Hp = s->Hp;
    Tally own;
    DevBuf<double> y, yt_all, rss_all, x, d_effect, d_se, d_lod, d_sigma2;
    DevBuf<int64_t> d_column, d_point;
    DevBuf<int32_t> d_rank;
    GBRS_TRY(own.alloc(y, (size_t)n * yc_max));
    GBRS_TRY(own.alloc(yt_all, (size_t)P * n_ld));
    GBRS_TRY(own.alloc(rss_all, (size_t)P));
    GBRS_TRY(own.alloc(x, (size_t)tc_max * Hp * n_ld));
    GBRS_TRY(own.alloc(d_effect, (size_t)tc_max * H));
    GBRS_TRY(own.alloc(d_se, (size_t)tc_max * H));
    GBRS_TRY(own.alloc(d_lod, (size_t)tc_max));
    GBRS_TRY(own.alloc(d_sigma2, (size_t)tc_max));
    GBRS_TRY(own.alloc(d_column, (size_t)tc_max));
    GBRS_TRY(own.alloc(d_point, (size_t)tc_max));
    GBRS_TRY(own.alloc(d_rank, (size_t)tc_max));
    GBRS_TRY(timed_open(s));
    GBRS_TRY(project_all(s, pr.qz, pr.c, n_ld, pheno, P, y, yt_all, rss_all));
    // the results of a chunk come to the host before the next chunk's kernel overwrites them: the stream orders the two
    std::vector<double> h_effect(effect ? (size_t)T * H : 0), h_se(se ? (size_t)T * H : 0), h_lod(lod ? (size_t)T : 0),
        h_sigma2(sigma2 ? (size_t)T : 0);
    std::vector<int32_t> h_rank(rank ? (size_t)T : 0);
    for (int64_t t0 = 0; t0 < T; t0 += SE_TCHUNK) {
        const int64_t tc = std::min(SE_TCHUNK, T - t0);
        GBRS_HIP_CHECK(hipMemcpyAsync(d_column.p, column + t0, (size_t)tc * sizeof(int64_t), hipMemcpyHostToDevice, s->stream));
        GBRS_HIP_CHECK(hipMemcpyAsync(d_point.p, point + t0, (size_t)tc * sizeof(int64_t), hipMemcpyHostToDevice, s->stream));
        auto launch = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, dim3((unsigned)tc), dim3(SC_THREADS), 0, s->stream, n, s->M, H, pr.c, n_ld, 0.5 * n, s->cohort.dosage.p,
                               pr.qz.p, pr.W.p, pr.d_rank.p, d_column.p, d_point.p, yt_all.p, rss_all.p, x.p, d_effect.p, d_se.p,
                               d_lod.p, d_sigma2.p, d_rank.p);
        };
        if (Hp == 8) launch(scan_effects_kernel<8>);
        else launch(scan_effects_kernel<16>);
        GBRS_HIP_CHECK(hipGetLastError());
        if (effect) GBRS_HIP_CHECK(hipMemcpyAsync(h_effect.data() + t0 * H, d_effect.p, (size_t)tc * H * sizeof(double), hipMemcpyDeviceToHost, s->stream));
        if (se) GBRS_HIP_CHECK(hipMemcpyAsync(h_se.data() + t0 * H, d_se.p, (size_t)tc * H * sizeof(double), hipMemcpyDeviceToHost, s->stream));
        if (lod) GBRS_HIP_CHECK(hipMemcpyAsync(h_lod.data() + t0, d_lod.p, (size_t)tc * sizeof(double), hipMemcpyDeviceToHost, s->stream));
        if (sigma2) GBRS_HIP_CHECK(hipMemcpyAsync(h_sigma2.data() + t0, d_sigma2.p, (size_t)tc * sizeof(double), hipMemcpyDeviceToHost, s->stream));
        if (rank) GBRS_HIP_CHECK(hipMemcpyAsync(h_rank.data() + t0, d_rank.p, (size_t)tc * sizeof(int32_t), hipMemcpyDeviceToHost, s->stream));
    }
    GBRS_TRY(timed_wait(s));
    // the caller's arrays are written once the whole pass has succeeded
    if (effect) std::memcpy(effect, h_effect.data(), h_effect.size() * sizeof(double));
    if (se) std::memcpy(se, h_se.data(), h_se.size() * sizeof(double));
    if (lod) std::memcpy(lod, h_lod.data(), h_lod.size() * sizeof(double));
    if (sigma2) std::memcpy(sigma2, h_sigma2.data(), h_sigma2.size() * sizeof(double));
    if (rank) std::memcpy(rank, h_rank.data(), h_rank.size() * sizeof(int32_t));
    gbrs_scan_effects_info_t &r = s->last.effects;
    r.T = T;
    r.P = P;
    r.last_pass_ms = pass_ms(s, r.last_pass_ms);
    r.peak_device_bytes = s->resident_bytes() + own.bytes;
    return GBRS_OK;
}

int gbrs_scan_effects_info(gbrs_scan_t *s, gbrs_scan_effects_info_t *info) {
    if (!s || !info) return fail(GBRS_ERR_INVALID, "bad argument");
    *info = s->last.effects;
    return GBRS_OK;
}

int gbrs_scan_info(gbrs_scan_t *s, gbrs_scan_info_t *info, int32_t *rank) {
    if (!s) return fail(GBRS_ERR_INVALID, "handle is NULL");
    if (info) {
        *info = s->last.scan;
        info->n = s->cohort.n;
        info->M = s->M;
        info->H = s->H;
        info->c = s->prep.c;
        info->device_bytes = s->scan_bytes();
    }
    if (rank && s->prep.c > 0) std::memcpy(rank, s->prep.rank.data(), s->prep.rank.size() * sizeof(int32_t));
    return GBRS_OK;
}

}  // extern "C"

// ---- linear mixed model ----------------------------------------------------------------------------------------

namespace {

// S_c of every chromosome, once per cohort: kept on the handle until the next append.
int scan_kinship_products(gbrs_scan *s) {
    if (s->kin.valid) return GBRS_OK;
    const int n = (int)s->cohort.n;
    const int64_t ld = s->M * s->H;
    GBRS_TRY(s->kin.S.alloc((size_t)s->n_chrom * n * n));
    bool vec2 = ld % 2 == 0;
    for (int c = 0; c < s->n_chrom; ++c) vec2 = vec2 && s->point_off[c] * s->H % 2 == 0;
    const unsigned blocks = (unsigned)((n + SC_ROWS - 1) / SC_ROWS);
    auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3(blocks, blocks, (unsigned)s->n_chrom), dim3(SC_THREADS), 0, s->stream, n, s->H, ld,
                           s->d_point_off.p, s->cohort.dosage.p, s->kin.S.p);
    };
    if (vec2) launch(lmm_kinship_kernel<true>);
    else launch(lmm_kinship_kernel<false>);
    GBRS_HIP_CHECK(hipGetLastError());
    s->kin.valid = true;
    return GBRS_OK;
}

// One launch of lmm_rotate_kernel: out [rows][n_ld] = (U' src)' on the handle's stream.
void scan_lmm_rotate(gbrs_scan *s, int64_t n_ld, int64_t rows, int HP, int keep, int64_t hs, int64_t ld_s, const double *U,
                     const double *src, double *out) {
    if (rows == 0) return;
    const dim3 grid((unsigned)((rows + 63) / 64), (unsigned)((n_ld + 63) / 64));
    hipLaunchKernelGGL(lmm_rotate_kernel, grid, dim3(SC_THREADS), 0, s->stream, (int)s->cohort.n, n_ld, rows, HP, keep, hs, ld_s, U, src,
                       out);
}

// One chunk of the mixed model's null fits, as its three passes share it: up to pc_max phenotype columns, their rotation by
// every decomposition and what lmm_null_kernel leaves for every (column, decomposition).  The buffers are the call's own.
struct LmmNull {
    DevBuf<double> y, ys, d_hin, d_hsq, d_sigma2, sw, qz, yt, rss0;
    DevBuf<int32_t> d_rmin, d_rmax;

    // d_hin only where the caller gives heritabilities
    int alloc(Tally &own, const gbrs_scan *s, int64_t pc_max, bool given) {
        const size_t pe = (size_t)pc_max * s->lmm.n_eig, n_ld = (size_t)s->lmm.n_ld;
        GBRS_TRY(own.alloc(y, (size_t)s->cohort.n * pc_max));
        GBRS_TRY(own.alloc(ys, pe * n_ld));
        if (given) GBRS_TRY(own.alloc(d_hin, pe));
        GBRS_TRY(own.alloc(d_hsq, pe));
        GBRS_TRY(own.alloc(d_sigma2, pe));
        GBRS_TRY(own.alloc(sw, pe * n_ld));
        GBRS_TRY(own.alloc(qz, pe * s->lmm.cz * n_ld));
        GBRS_TRY(own.alloc(yt, pe * n_ld));
        GBRS_TRY(own.alloc(rss0, pe));
        GBRS_TRY(own.alloc(d_rmin, (size_t)pc_max));
        GBRS_TRY(own.alloc(d_rmax, (size_t)pc_max));
        return GBRS_OK;
    }

    // Columns [p0, p0 + pc) of the host table [n][ld], with their rows of hsq_in [ld][n_eig] where given: uploads,
    // rotations, lmm_null_kernel.  The passes time this differently (gbrs_hip.h), so each brings its events, both
    // nullable: `uploaded` is recorded before the rotations and `rotated` before the null kernel; the end is the caller's.
    int fit(gbrs_scan *s, const double *table, int64_t ld, const double *hsq_in, int64_t p0, int64_t pc, hipEvent_t uploaded,
            hipEvent_t rotated) {
        const gbrs_scan::Lmm &lm = s->lmm;
        const int n = (int)s->cohort.n;
        GBRS_TRY(upload_columns(s, y, table, ld, p0, pc));
        if (hsq_in)
            GBRS_HIP_CHECK(hipMemcpyAsync(d_hin.p, hsq_in + p0 * lm.n_eig, (size_t)pc * lm.n_eig * sizeof(double), hipMemcpyHostToDevice, s->stream));
        if (uploaded) GBRS_HIP_CHECK(hipEventRecord(uploaded, s->stream));
        for (int e = 0; e < lm.n_eig; ++e)
            scan_lmm_rotate(s, lm.n_ld, pc, 1, 1, 1, pc, lm.U.p + (size_t)e * n * n, y.p, ys.p + (size_t)e * pc * lm.n_ld);
        if (rotated) GBRS_HIP_CHECK(hipEventRecord(rotated, s->stream));
        hipLaunchKernelGGL(lmm_null_kernel, dim3((unsigned)pc, (unsigned)lm.n_eig), dim3(64), 0, s->stream, n, lm.cz, lm.n_ld, pc, lm.n_eig,
                           ys.p, lm.Zs.p, lm.lam.p, d_hin.p, d_hsq.p, d_sigma2.p, sw.p, qz.p, yt.p, rss0.p, d_rmin.p, d_rmax.p);
        return GBRS_OK;
    }
};

// The weighted columns [Hp][n_ld] of a point or of a target: the workgroup's LDS, or past LM_LDS_BYTES a workspace of the
// call's own with one slice per workgroup in flight.
struct LmmWeighted {
    size_t w_bytes;
    bool in_lds;
    DevBuf<double> ws;                        // stays empty, and its pointer null, with in_lds
    explicit LmmWeighted(const gbrs_scan *s) : w_bytes((size_t)s->Hp * s->lmm.n_ld * sizeof(double)), in_lds(w_bytes <= LM_LDS_BYTES) {}
    int alloc(Tally &own, int64_t slices) { return in_lds ? GBRS_OK : own.alloc(ws, (size_t)slices * (w_bytes / sizeof(double))); }
    size_t lds_bytes() const { return in_lds ? w_bytes : 0; }
};

}  // namespace

extern "C" {

int gbrs_scan_kinship(gbrs_scan_t *s, int leave_out, double scale, double *K) {
    RoctxRange roctx_range("gbrs_scan_kinship");
    if (!s) return fail(GBRS_ERR_INVALID, "handle is NULL");
    if (!K) return fail(GBRS_ERR_INVALID, "K is NULL");
    const int64_t n = s->cohort.n;
    if (n < 1) return fail(GBRS_ERR_INVALID, "the cohort has no samples");
    if (n > LM_MAX_N) return fail(GBRS_ERR_INVALID, "a kinship takes at most %d samples, the cohort has %lld", LM_MAX_N, (long long)n);
    if (leave_out < -1 || leave_out >= s->n_chrom)
        return fail(GBRS_ERR_INVALID, "chromosome %d to leave out is not one of the handle's %d (-1: none)", leave_out, s->n_chrom);
    if (!std::isfinite(scale)) return fail(GBRS_ERR_INVALID, "the kinship's scale is not finite");
    int64_t count = 0;
    for (int c = 0; c < s->n_chrom; ++c)
        if (c != leave_out) count += s->points[c];
    if (count == 0)
        return fail(GBRS_ERR_INVALID, "chromosome %d holds every grid point: its leave-one-chromosome-out kinship has nothing to be formed from", leave_out);
    GBRS_TRY(select_device(s->device));
    const int64_t nn = n * n;
    DevBuf<double> d_K;
    GBRS_TRY(d_K.alloc((size_t)nn));
    GBRS_TRY(timed_open(s));
    GBRS_TRY(scan_kinship_products(s));
    hipLaunchKernelGGL(lmm_kinship_sum_kernel, dim3((unsigned)((nn + 255) / 256)), dim3(256), 0, s->stream, nn, s->n_chrom, leave_out,
                       scale, (double)count, s->kin.S.p, d_K.p);
    GBRS_HIP_CHECK(hipEventRecord(s->ev[1], s->stream));
    GBRS_HIP_CHECK(hipGetLastError());
    const hipError_t done = hipStreamSynchronize(s->stream);     // not timed_wait: a failure here takes the products with it
    if (done != hipSuccess) {
        s->kin.valid = false;
        return fail(GBRS_ERR_HIP, "the kinship kernels failed: %s", hipGetErrorString(done));
    }
    s->last.lmm.last_kinship_ms = pass_ms(s, s->last.lmm.last_kinship_ms);
    GBRS_TRY(copy_out(K, d_K, d_K.n));
    return GBRS_OK;
}

int gbrs_scan_lmm_prepare(gbrs_scan_t *s, int cz, const double *Z, int n_eig, const double *const *U, const double *const *lambda,
                          const int32_t *eig_of_chrom) {
    RoctxRange roctx_range("gbrs_scan_lmm_prepare");
    if (!s) return fail(GBRS_ERR_INVALID, "handle is NULL");
    if (cz < 1 || cz > LM_MAX_C)
        return fail(GBRS_ERR_INVALID, "covariate columns of the mixed model must be 1..%d (the intercept included), got %d", LM_MAX_C, cz);
    if (!Z || !U || !lambda || !eig_of_chrom) return fail(GBRS_ERR_INVALID, "bad argument");
    if (n_eig < 1 || n_eig > s->n_chrom)
        return fail(GBRS_ERR_INVALID, "the decompositions must number 1..%d (one per chromosome at most), got %d", s->n_chrom, n_eig);
    if (s->cohort.n <= (int64_t)cz + s->H - 1)
        return fail(GBRS_ERR_INVALID, "%lld samples are too few for %d covariate columns and %d founders: need more than %d",
                    (long long)s->cohort.n, cz, s->H, cz + s->H - 1);
    if (s->cohort.n > LM_MAX_N)
        return fail(GBRS_ERR_INVALID, "the mixed model takes at most %d samples, the cohort has %lld", LM_MAX_N, (long long)s->cohort.n);
    const int n = (int)s->cohort.n;
    for (int c = 0; c < s->n_chrom; ++c)
        if (eig_of_chrom[c] < 0 || eig_of_chrom[c] >= n_eig)
            return fail(GBRS_ERR_INVALID, "chromosome %d is mapped to decomposition %d of %d", c, eig_of_chrom[c], n_eig);
    for (int64_t k = 0; k < (int64_t)n * cz; ++k)
        if (!std::isfinite(Z[k]))
            return fail(GBRS_ERR_INVALID, "covariates hold a value that is not finite (sample %lld, column %d)", (long long)(k / cz), (int)(k % cz));
    for (int e = 0; e < n_eig; ++e) {
        if (!U[e] || !lambda[e]) return fail(GBRS_ERR_INVALID, "decomposition %d is NULL", e);
        double top = 0.0;
        for (int i = 0; i < n; ++i) {
            if (!std::isfinite(lambda[e][i]))
                return fail(GBRS_ERR_INVALID, "decomposition %d: eigenvalue %d is not finite", e, i);
            top = std::max(top, lambda[e][i]);
        }
        for (int i = 0; i < n; ++i)
            if (!(lambda[e][i] > LM_LAMBDA * top))
                return fail(GBRS_ERR_INVALID, "decomposition %d: eigenvalue %d is %g, not above %g of the largest (%g): the kinship is "
                            "singular - the cohort has fewer independent dosage columns than samples", e, i, lambda[e][i], LM_LAMBDA, top);
        for (int64_t k = 0; k < (int64_t)n * n; ++k)
            if (!std::isfinite(U[e][k]))
                return fail(GBRS_ERR_INVALID, "decomposition %d: the eigenvectors hold a value that is not finite (row %lld, column %lld)", e,
                            (long long)(k / n), (long long)(k % n));
    }
    GBRS_TRY(select_device(s->device));
    // staged in the call's own buffers: an earlier preparation stands until everything below has succeeded
    const int64_t n_ld = padded(n);
    DevBuf<double> d_U, d_lam, d_Z, d_Zs, d_R;
    DevBuf<int32_t> d_eop;
    GBRS_TRY(d_U.alloc((size_t)n_eig * n * n));
    GBRS_TRY(d_lam.alloc((size_t)n_eig * n));
    GBRS_TRY(d_Z.alloc((size_t)n * cz));
    GBRS_TRY(d_Zs.alloc((size_t)n_eig * cz * n_ld));
    GBRS_TRY(d_R.alloc((size_t)s->M * s->Hp * n_ld));
    GBRS_TRY(d_eop.alloc((size_t)s->M));
    std::vector<int32_t> eop((size_t)s->M);
    for (int c = 0; c < s->n_chrom; ++c)
        for (int64_t m = s->point_off[c]; m < s->point_off[c + 1]; ++m) eop[m] = eig_of_chrom[c];
    for (int e = 0; e < n_eig; ++e) {
        GBRS_HIP_CHECK(hipMemcpy(d_U.p + (size_t)e * n * n, U[e], (size_t)n * n * sizeof(double), hipMemcpyHostToDevice));
        GBRS_HIP_CHECK(hipMemcpy(d_lam.p + (size_t)e * n, lambda[e], (size_t)n * sizeof(double), hipMemcpyHostToDevice));
    }
    GBRS_HIP_CHECK(hipMemcpy(d_Z.p, Z, d_Z.bytes(), hipMemcpyHostToDevice));
    GBRS_HIP_CHECK(hipMemcpy(d_eop.p, eop.data(), d_eop.bytes(), hipMemcpyHostToDevice));
    GBRS_TRY(timed_open(s));
    for (int e = 0; e < n_eig; ++e)
        scan_lmm_rotate(s, n_ld, cz, 1, 1, 1, cz, d_U.p + (size_t)e * n * n, d_Z.p, d_Zs.p + (size_t)e * cz * n_ld);
    for (int c = 0; c < s->n_chrom; ++c)
        scan_lmm_rotate(s, n_ld, (int64_t)s->points[c] * s->Hp, s->Hp, s->H - 1, s->H, s->M * s->H,
                        d_U.p + (size_t)eig_of_chrom[c] * n * n, s->cohort.dosage.p + s->point_off[c] * s->H,
                        d_R.p + s->point_off[c] * s->Hp * n_ld);
    GBRS_TRY(timed_wait(s));
    s->last.lmm.last_rotate_ms = pass_ms(s, s->last.lmm.last_rotate_ms);
    gbrs_scan::Lmm &lm = s->lmm;
    lm.U.swap(d_U);
    lm.lam.swap(d_lam);
    lm.Zs.swap(d_Zs);
    lm.R.swap(d_R);
    lm.eig_of_point.swap(d_eop);
    lm.eig_of_chrom.assign(eig_of_chrom, eig_of_chrom + s->n_chrom);
    lm.cz = cz;
    lm.n_eig = n_eig;
    lm.n_ld = n_ld;
    return GBRS_OK;
}

}  // extern "C"

namespace {

// The pass of gbrs_scan_lmm_run.  With support, gbrs_scan_lmm_run_support's: the intervals of every chunk follow its peaks
// while its LOD rows are on the device, by scan_run_pass' kernel; the two tables of a chunk are the call's own.
int scan_lmm_run_pass(gbrs_scan *s, int64_t P, const double *pheno, const double *hsq_in, bool support, double drop, double *lod,
                      double *peak_lod, int64_t *peak_index, double *hsq, double *sigma2, int64_t *support_lo,
                      int64_t *support_hi) {
    if (!s) return fail(GBRS_ERR_INVALID, "handle is NULL");
    if (s->lmm.cz == 0) return fail(GBRS_ERR_INVALID, "no mixed model on the handle: call gbrs_scan_lmm_prepare first");
    if (P < 1 || !pheno) return fail(GBRS_ERR_INVALID, "bad argument");
    if (support && !(drop >= 0.0 && std::isfinite(drop)))
        return fail(GBRS_ERR_INVALID, "the LOD drop of a support interval must be a finite number that is not negative, got %g", drop);
    gbrs_scan::Lmm &lm = s->lmm;
    const int n = (int)s->cohort.n, cz = lm.cz, n_eig = lm.n_eig, nc = s->n_chrom;
    GBRS_TRY(check_finite("phenotype", pheno, n, P));
    GBRS_TRY(check_hsq(hsq_in, P, n_eig));
    GBRS_TRY(select_device(s->device));
    const int64_t pc_max = std::min(P, SC_PCHUNK), M = s->M, n_ld = lm.n_ld;
    const int Hp = s->Hp;
    Tally own;
    LmmNull null;
    DevBuf<double> d_lod, d_peak;
    DevBuf<int64_t> d_index, d_lo, d_hi;
    GBRS_TRY(null.alloc(own, s, pc_max, hsq_in != nullptr));
    GBRS_TRY(own.alloc(d_lod, (size_t)pc_max * M));
    GBRS_TRY(own.alloc(d_peak, (size_t)pc_max * nc));
    GBRS_TRY(own.alloc(d_index, (size_t)pc_max * nc));
    if (support) {
        GBRS_TRY(own.alloc(d_lo, (size_t)pc_max * nc));
        GBRS_TRY(own.alloc(d_hi, (size_t)pc_max * nc));
    }
    // past LM_LDS_BYTES the points go in batches through the workspace
    LmmWeighted wc(s);
    const int64_t tiles_max = (pc_max + LM_TILE - 1) / LM_TILE;
    const int64_t batch = wc.in_lds ? M : std::max<int64_t>(1, std::min<int64_t>(M, (int64_t)(LM_WS_BYTES / (wc.w_bytes * tiles_max))));
    GBRS_TRY(wc.alloc(own, batch * tiles_max));
    std::vector<int32_t> rmin((size_t)P), rmax((size_t)P);
    double t_null = 0.0, t_point = 0.0;
    Marks mark;
    GBRS_TRY(mark.create());
    GBRS_TRY(timed_open(s));
    for (int64_t p0 = 0; p0 < P; p0 += SC_PCHUNK) {
        const int64_t pc = std::min(SC_PCHUNK, P - p0);
        const size_t peaks = (size_t)pc * nc, fits = (size_t)pc * n_eig;
        GBRS_TRY(null.fit(s, pheno, P, hsq_in, p0, pc, nullptr, mark.ev[0]));        // last_null_ms: the null kernel alone
        GBRS_HIP_CHECK(hipEventRecord(mark.ev[1], s->stream));
        const unsigned tiles = (unsigned)((pc + LM_TILE - 1) / LM_TILE);
        for (int64_t m0 = 0; m0 < M; m0 += batch) {
            const dim3 grid((unsigned)std::min(batch, M - m0), tiles);
            auto launch = [&](auto kernel) {
                hipLaunchKernelGGL(kernel, grid, dim3(SC_THREADS), wc.lds_bytes(), s->stream, n, M, m0, s->H, cz, n_ld, pc, n_eig, LM_TILE,
                                   0.5 * n, lm.eig_of_point.p, lm.R.p, null.sw.p, null.qz.p, null.yt.p, null.rss0.p, wc.ws.p, d_lod.p,
                                   null.d_rmin.p, null.d_rmax.p);
            };
            if (Hp == 8) launch(lmm_point_kernel<8>);
            else launch(lmm_point_kernel<16>);
        }
        GBRS_HIP_CHECK(hipEventRecord(mark.ev[2], s->stream));
        hipLaunchKernelGGL(scan_peak_kernel, dim3((unsigned)nc, (unsigned)pc), dim3(64), 0, s->stream, M, nc, s->d_point_off.p, d_lod.p,
                           d_peak.p, d_index.p);
        if (support)
            hipLaunchKernelGGL(scan_support_kernel, dim3((unsigned)nc, (unsigned)pc), dim3(64), 0, s->stream, M, nc, drop,
                               s->d_point_off.p, d_lod.p, d_peak.p, d_index.p, d_lo.p, d_hi.p);
        GBRS_HIP_CHECK(hipGetLastError());
        GBRS_HIP_CHECK(hipStreamSynchronize(s->stream));
        t_null += elapsed_ms(mark.ev[0], mark.ev[1], 0.0);
        t_point += elapsed_ms(mark.ev[1], mark.ev[2], 0.0);
        GBRS_TRY(copy_out(lod, d_lod, (size_t)pc * M, (size_t)p0 * M));
        GBRS_TRY(copy_out(peak_lod, d_peak, peaks, (size_t)p0 * nc));
        GBRS_TRY(copy_out(peak_index, d_index, peaks, (size_t)p0 * nc));
        GBRS_TRY(copy_out(hsq, null.d_hsq, fits, (size_t)p0 * n_eig));
        GBRS_TRY(copy_out(sigma2, null.d_sigma2, fits, (size_t)p0 * n_eig));
        GBRS_TRY(copy_out(support_lo, d_lo, peaks, (size_t)p0 * nc));
        GBRS_TRY(copy_out(support_hi, d_hi, peaks, (size_t)p0 * nc));
        GBRS_TRY(copy_out(rmin.data(), null.d_rmin, (size_t)pc, (size_t)p0));
        GBRS_TRY(copy_out(rmax.data(), null.d_rmax, (size_t)pc, (size_t)p0));
    }
    GBRS_TRY(timed_wait(s));
    gbrs_scan_lmm_info_t &r = s->last.lmm;
    r.P = P;
    r.last_run_ms = pass_ms(s, r.last_run_ms);
    r.last_null_ms = t_null;
    r.last_point_ms = t_point;
    r.peak_device_bytes = s->resident_bytes() + own.bytes;
    lm.rank_min.swap(rmin);
    lm.rank_max.swap(rmax);
    return GBRS_OK;
}

}  // namespace

extern "C" {

int gbrs_scan_lmm_run(gbrs_scan_t *s, int64_t P, const double *pheno, const double *hsq_in, double *lod, double *peak_lod,
                      int64_t *peak_index, double *hsq, double *sigma2) {
    RoctxRange roctx_range("gbrs_scan_lmm_run");
    return scan_lmm_run_pass(s, P, pheno, hsq_in, false, 0.0, lod, peak_lod, peak_index, hsq, sigma2, nullptr, nullptr);
}

int gbrs_scan_lmm_run_support(gbrs_scan_t *s, int64_t P, const double *pheno, const double *hsq_in, double drop, double *lod,
                              double *peak_lod, int64_t *peak_index, double *hsq, double *sigma2, int64_t *support_lo,
                              int64_t *support_hi) {
    RoctxRange roctx_range("gbrs_scan_lmm_run_support");
    return scan_lmm_run_pass(s, P, pheno, hsq_in, true, drop, lod, peak_lod, peak_index, hsq, sigma2, support_lo, support_hi);
}

// Founder effects under the mixed model.  The columns some target names are compacted on the host and pass
// in gbrs_scan_lmm_run's chunks of 512 through its rotation and its null fits - every decomposition of a used column, hsq_in
// honoured -; a chunk's targets, in the caller's order, follow in chunks of SE_TCHUNK while the chunk's fits are on the device.
int gbrs_scan_lmm_effects(gbrs_scan_t *s, int64_t P, const double *pheno, const double *hsq_in, int64_t T, const int64_t *column,
                          const int64_t *point, double *effect, double *se, double *lod, double *sigma2, int32_t *rank,
                          double *hsq) {
    RoctxRange roctx_range("gbrs_scan_lmm_effects");
    if (!s) return fail(GBRS_ERR_INVALID, "handle is NULL");
    if (s->lmm.cz == 0) return fail(GBRS_ERR_INVALID, "no mixed model on the handle: call gbrs_scan_lmm_prepare first");
    if (P < 1) return fail(GBRS_ERR_INVALID, "an effects pass needs at least 1 phenotype, got %lld", (long long)P);
    if (T < 0) return fail(GBRS_ERR_INVALID, "the number of targets cannot be negative, got %lld", (long long)T);
    if (!pheno || (T > 0 && (!column || !point))) return fail(GBRS_ERR_INVALID, "bad argument");
    const gbrs_scan::Lmm &lm = s->lmm;
    const int n = (int)s->cohort.n, cz = lm.cz, n_eig = lm.n_eig, H = s->H, Hp = s->Hp;
    GBRS_TRY(check_targets(s, T, column, P, point));
    GBRS_TRY(check_finite("phenotype", pheno, n, P));
    GBRS_TRY(check_hsq(hsq_in, P, n_eig));
    if (T == 0) return GBRS_OK;
    // the used columns in ascending order, and every column's targets in the caller's order
    std::vector<int64_t> slot((size_t)P, -1), used;
    for (int64_t t = 0; t < T; ++t) slot[column[t]] = 0;
    for (int64_t p = 0; p < P; ++p)
        if (slot[p] == 0) {
            slot[p] = (int64_t)used.size();
            used.push_back(p);
        }
    const int64_t Pu = (int64_t)used.size(), pc_max = std::min(Pu, SC_PCHUNK), n_ld = lm.n_ld;
    std::vector<double> y_used((size_t)n * Pu), h_used(hsq_in ? (size_t)Pu * n_eig : 0);
    for (int64_t i = 0; i < n; ++i)
        for (int64_t q = 0; q < Pu; ++q) y_used[i * Pu + q] = pheno[i * P + used[q]];
    if (hsq_in)
        for (int64_t q = 0; q < Pu; ++q)
            for (int e = 0; e < n_eig; ++e) h_used[q * n_eig + e] = hsq_in[used[q] * n_eig + e];
    std::vector<std::vector<int64_t>> of_chunk((size_t)((Pu + SC_PCHUNK - 1) / SC_PCHUNK));
    for (int64_t t = 0; t < T; ++t) of_chunk[slot[column[t]] / SC_PCHUNK].push_back(t);
    GBRS_TRY(select_device(s->device));
    const int64_t tc_max = std::min(T, SE_TCHUNK);
    Tally own;
    LmmNull null;
    DevBuf<double> d_effect, d_se, d_lod, d_sigma2, d_hout;
    DevBuf<int64_t> d_column, d_point;
    DevBuf<int32_t> d_rank;
    GBRS_TRY(null.alloc(own, s, pc_max, hsq_in != nullptr));
    GBRS_TRY(own.alloc(d_effect, (size_t)tc_max * H));
    GBRS_TRY(own.alloc(d_se, (size_t)tc_max * H));
    GBRS_TRY(own.alloc(d_lod, (size_t)tc_max));
    GBRS_TRY(own.alloc(d_sigma2, (size_t)tc_max));
    GBRS_TRY(own.alloc(d_hout, (size_t)tc_max));
    GBRS_TRY(own.alloc(d_rank, (size_t)tc_max));
    GBRS_TRY(own.alloc(d_column, (size_t)tc_max));
    GBRS_TRY(own.alloc(d_point, (size_t)tc_max));
    LmmWeighted wc(s);                  // past LM_LDS_BYTES a target has its slice of the workspace
    GBRS_TRY(wc.alloc(own, tc_max));
    std::vector<double> h_effect((size_t)T * H), h_se((size_t)T * H), h_lod((size_t)T), h_sigma2((size_t)T), h_hsq((size_t)T);
    std::vector<int32_t> h_rank((size_t)T);
    std::vector<double> c_effect((size_t)tc_max * H), c_se((size_t)tc_max * H), c_lod((size_t)tc_max), c_sigma2((size_t)tc_max),
        c_hsq((size_t)tc_max);
    std::vector<int32_t> c_rank((size_t)tc_max);
    std::vector<int64_t> c_column((size_t)tc_max), c_point((size_t)tc_max);
    double t_null = 0.0, t_target = 0.0;
    Marks mark;
    GBRS_TRY(mark.create());
    GBRS_TRY(timed_open(s));
    for (int64_t p0 = 0; p0 < Pu; p0 += SC_PCHUNK) {
        const int64_t pc = std::min(SC_PCHUNK, Pu - p0);
        const std::vector<int64_t> &mine = of_chunk[(size_t)(p0 / SC_PCHUNK)];
        GBRS_TRY(null.fit(s, y_used.data(), Pu, hsq_in ? h_used.data() : nullptr, p0, pc, mark.ev[0], nullptr));  // last_null_ms: rotations and REML
        GBRS_HIP_CHECK(hipEventRecord(mark.ev[1], s->stream));
        GBRS_HIP_CHECK(hipGetLastError());
        for (size_t t0 = 0; t0 < mine.size(); t0 += (size_t)SE_TCHUNK) {
            const int64_t tc = (int64_t)std::min<size_t>((size_t)SE_TCHUNK, mine.size() - t0);
            for (int64_t k = 0; k < tc; ++k) {
                const int64_t t = mine[t0 + k];
                c_column[k] = slot[column[t]] - p0;
                c_point[k] = point[t];
            }
            GBRS_HIP_CHECK(hipMemcpyAsync(d_column.p, c_column.data(), (size_t)tc * sizeof(int64_t), hipMemcpyHostToDevice, s->stream));
            GBRS_HIP_CHECK(hipMemcpyAsync(d_point.p, c_point.data(), (size_t)tc * sizeof(int64_t), hipMemcpyHostToDevice, s->stream));
            auto launch = [&](auto kernel) {
                hipLaunchKernelGGL(kernel, dim3((unsigned)tc), dim3(SC_THREADS), wc.lds_bytes(), s->stream, n, H, cz, n_ld, n_eig, 0.5 * n,
                                   lm.eig_of_point.p, lm.R.p, null.sw.p, null.qz.p, null.yt.p, null.rss0.p, null.d_hsq.p, d_column.p,
                                   d_point.p, wc.ws.p, d_effect.p, d_se.p, d_lod.p, d_sigma2.p, d_rank.p, d_hout.p);
            };
            if (Hp == 8) launch(lmm_effects_kernel<8>);
            else launch(lmm_effects_kernel<16>);
            GBRS_HIP_CHECK(hipGetLastError());
            GBRS_HIP_CHECK(hipMemcpyAsync(c_effect.data(), d_effect.p, (size_t)tc * H * sizeof(double), hipMemcpyDeviceToHost, s->stream));
            GBRS_HIP_CHECK(hipMemcpyAsync(c_se.data(), d_se.p, (size_t)tc * H * sizeof(double), hipMemcpyDeviceToHost, s->stream));
            GBRS_HIP_CHECK(hipMemcpyAsync(c_lod.data(), d_lod.p, (size_t)tc * sizeof(double), hipMemcpyDeviceToHost, s->stream));
            GBRS_HIP_CHECK(hipMemcpyAsync(c_sigma2.data(), d_sigma2.p, (size_t)tc * sizeof(double), hipMemcpyDeviceToHost, s->stream));
            GBRS_HIP_CHECK(hipMemcpyAsync(c_hsq.data(), d_hout.p, (size_t)tc * sizeof(double), hipMemcpyDeviceToHost, s->stream));
            GBRS_HIP_CHECK(hipMemcpyAsync(c_rank.data(), d_rank.p, (size_t)tc * sizeof(int32_t), hipMemcpyDeviceToHost, s->stream));
            GBRS_HIP_CHECK(hipStreamSynchronize(s->stream));
            for (int64_t k = 0; k < tc; ++k) {              // to the target's own place
                const int64_t t = mine[t0 + k];
                std::memcpy(h_effect.data() + t * H, c_effect.data() + k * H, (size_t)H * sizeof(double));
                std::memcpy(h_se.data() + t * H, c_se.data() + k * H, (size_t)H * sizeof(double));
                h_lod[t] = c_lod[k];
                h_sigma2[t] = c_sigma2[k];
                h_hsq[t] = c_hsq[k];
                h_rank[t] = c_rank[k];
            }
        }
        GBRS_HIP_CHECK(hipEventRecord(mark.ev[2], s->stream));
        GBRS_HIP_CHECK(hipStreamSynchronize(s->stream));
        t_null += elapsed_ms(mark.ev[0], mark.ev[1], 0.0);
        t_target += elapsed_ms(mark.ev[1], mark.ev[2], 0.0);
    }
    GBRS_TRY(timed_wait(s));
    // the caller's arrays are written once the whole pass has succeeded
    if (effect) std::memcpy(effect, h_effect.data(), h_effect.size() * sizeof(double));
    if (se) std::memcpy(se, h_se.data(), h_se.size() * sizeof(double));
    if (lod) std::memcpy(lod, h_lod.data(), h_lod.size() * sizeof(double));
    if (sigma2) std::memcpy(sigma2, h_sigma2.data(), h_sigma2.size() * sizeof(double));
    if (rank) std::memcpy(rank, h_rank.data(), h_rank.size() * sizeof(int32_t));
    if (hsq) std::memcpy(hsq, h_hsq.data(), h_hsq.size() * sizeof(double));
    gbrs_scan_lmm_effects_info_t &r = s->last.lmm_effects;
    r.T = T;
    r.P = P;
    r.columns = Pu;
    r.last_pass_ms = pass_ms(s, r.last_pass_ms);
    r.last_null_ms = t_null;
    r.last_target_ms = t_target;
    r.peak_device_bytes = s->resident_bytes() + own.bytes;
    return GBRS_OK;
}

int gbrs_scan_lmm_effects_info(gbrs_scan_t *s, gbrs_scan_lmm_effects_info_t *info) {
    if (!s || !info) return fail(GBRS_ERR_INVALID, "bad argument");
    *info = s->last.lmm_effects;
    return GBRS_OK;
}

int gbrs_scan_lmm_ranks(gbrs_scan_t *s, int32_t *rank_min, int32_t *rank_max) {
    if (!s) return fail(GBRS_ERR_INVALID, "handle is NULL");
    if (rank_min) std::memcpy(rank_min, s->lmm.rank_min.data(), s->lmm.rank_min.size() * sizeof(int32_t));
    if (rank_max) std::memcpy(rank_max, s->lmm.rank_max.data(), s->lmm.rank_max.size() * sizeof(int32_t));
    return GBRS_OK;
}

int gbrs_scan_lmm_info(gbrs_scan_t *s, gbrs_scan_lmm_info_t *info) {
    if (!s || !info) return fail(GBRS_ERR_INVALID, "bad argument");
    *info = s->last.lmm;
    info->cz = s->lmm.cz;
    info->n_eig = s->lmm.n_eig;
    info->device_bytes = s->kin.S.bytes() + s->lmm.bytes();
    return GBRS_OK;
}

// SNP association under the mixed model.  Two phases on the handle's stream: the null fits of every
// phenotype by gbrs_scan_lmm_run's kernels in its chunks of 512, their weighted columns kept on the device for all P;
// then the SNP chunks, each one's dosages formed and rotated once and multiplied with every phenotype chunk's columns.
int gbrs_scan_lmm_snps(gbrs_scan_t *s, int64_t P, const double *pheno, const double *hsq_in, double *lod, uint8_t *used,
                       double *peak_lod, int64_t *peak_index, int64_t *n_used, double *hsq, double *sigma2) {
    RoctxRange roctx_range("gbrs_scan_lmm_snps");
    if (!s) return fail(GBRS_ERR_INVALID, "handle is NULL");
    if (s->snp.M == 0) return fail(GBRS_ERR_INVALID, "no SNPs on the handle: call gbrs_scan_set_snps first");
    if (s->lmm.cz == 0) return fail(GBRS_ERR_INVALID, "no mixed model on the handle: call gbrs_scan_lmm_prepare first");
    if (P < 1) return fail(GBRS_ERR_INVALID, "a SNP pass needs at least 1 phenotype, got %lld", (long long)P);
    if (!pheno) return fail(GBRS_ERR_INVALID, "bad argument");
    const gbrs_scan::Lmm &lm = s->lmm;
    const gbrs_scan::Snp &sn = s->snp;
    const int n = (int)s->cohort.n, cz = lm.cz, n_eig = lm.n_eig, nc = s->n_chrom;
    GBRS_TRY(check_finite("phenotype", pheno, n, P));
    GBRS_TRY(check_hsq(hsq_in, P, n_eig));
    GBRS_TRY(select_device(s->device));
    int lds_max = 0;
    GBRS_HIP_CHECK(hipDeviceGetAttribute(&lds_max, hipDeviceAttributeMaxSharedMemoryPerBlock, s->device));
    if ((size_t)lds_max < LS_LDS_BYTES)
        return fail(GBRS_ERR_INVALID, "the device gives a workgroup %d bytes of LDS, the SNP product needs %lld", lds_max, (long long)LS_LDS_BYTES);
    GBRS_HIP_CHECK(hipFuncSetAttribute(reinterpret_cast<const void *>(lmm_snp_lod_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)LS_LDS_BYTES));
    const int64_t M_snp = sn.M, n_ld = lm.n_ld, pc_max = std::min(P, SC_PCHUNK), lc_max = std::min(M_snp, SS_CHUNK);
    const int64_t q_stride = P * n_ld;
    Tally own;
    LmmNull null;
    DevBuf<double> cols, rss_all, dose, xs, d_lod, d_peak;
    DevBuf<int64_t> d_index, d_count;
    DevBuf<uint8_t> d_used;
    GBRS_TRY(null.alloc(own, s, pc_max, hsq_in != nullptr));
    GBRS_TRY(own.alloc(cols, (size_t)n_eig * (cz + 2) * q_stride));
    GBRS_TRY(own.alloc(rss_all, (size_t)n_eig * P));
    GBRS_TRY(own.alloc(dose, (size_t)n * lc_max));
    GBRS_TRY(own.alloc(xs, (size_t)lc_max * n_ld));
    GBRS_TRY(own.alloc(d_lod, (size_t)pc_max * lc_max));
    GBRS_TRY(own.alloc(d_used, (size_t)pc_max * lc_max));
    GBRS_TRY(own.alloc(d_peak, (size_t)P * nc));
    GBRS_TRY(own.alloc(d_index, (size_t)P * nc));
    GBRS_TRY(own.alloc(d_count, (size_t)P * nc));
    EventRing null_ring, rotate_ring, product_ring;
    GBRS_TRY(null_ring.create());
    GBRS_TRY(rotate_ring.create());
    GBRS_TRY(product_ring.create());
    int slot = 0;
    GBRS_TRY(timed_open(s));
    GBRS_HIP_CHECK(hipMemsetAsync(d_index.p, 0xFF, d_index.bytes(), s->stream));         // -1: nothing yet
    GBRS_HIP_CHECK(hipMemsetAsync(d_count.p, 0, d_count.bytes(), s->stream));
    for (int64_t p0 = 0; p0 < P; p0 += SC_PCHUNK) {
        const int64_t pc = std::min(SC_PCHUNK, P - p0);
        GBRS_TRY(null_ring.next(&slot));
        GBRS_TRY(null.fit(s, pheno, P, hsq_in, p0, pc, null_ring.ev[2 * slot], nullptr));    // last_null_ms: rotations, REML, the columns
        hipLaunchKernelGGL(lmm_snp_column_kernel, dim3((unsigned)((pc * n_eig * n_ld + SC_THREADS - 1) / SC_THREADS)), dim3(SC_THREADS), 0,
                           s->stream, n_ld, pc, p0, P, n_eig, cz, null.sw.p, null.qz.p, null.yt.p, null.rss0.p, cols.p, rss_all.p);
        GBRS_HIP_CHECK(hipEventRecord(null_ring.ev[2 * slot + 1], s->stream));
        GBRS_HIP_CHECK(hipGetLastError());
        // waits for the kernels before it on the stream; the next chunk's null fit overwrites the two tables after it
        if (hsq)
            GBRS_HIP_CHECK(hipMemcpyAsync(hsq + p0 * n_eig, null.d_hsq.p, (size_t)pc * n_eig * sizeof(double), hipMemcpyDeviceToHost, s->stream));
        if (sigma2)
            GBRS_HIP_CHECK(hipMemcpyAsync(sigma2 + p0 * n_eig, null.d_sigma2.p, (size_t)pc * n_eig * sizeof(double), hipMemcpyDeviceToHost, s->stream));
    }
    for (int64_t j0 = 0; j0 < M_snp; j0 += SS_CHUNK) {
        const int64_t jc = std::min(SS_CHUNK, M_snp - j0);
        // the runs of the chunk's SNPs that share a decomposition: [first, second) in the chunk, chromosome after chromosome
        std::vector<std::pair<int64_t, int64_t>> runs;
        std::vector<int> run_eig;
        for (int c = 0; c < nc; ++c) {
            const int64_t a = std::max(sn.off[c], j0) - j0, b = std::min(sn.off[c + 1], j0 + jc) - j0;
            if (a >= b) continue;
            if (!runs.empty() && run_eig.back() == lm.eig_of_chrom[c]) runs.back().second = b;
            else {
                runs.emplace_back(a, b);
                run_eig.push_back(lm.eig_of_chrom[c]);
            }
        }
        GBRS_TRY(rotate_ring.next(&slot));
        GBRS_HIP_CHECK(hipEventRecord(rotate_ring.ev[2 * slot], s->stream));
        hipLaunchKernelGGL(scan_snp_dosage_kernel, dim3((unsigned)((n * jc + SC_THREADS - 1) / SC_THREADS)), dim3(SC_THREADS), 0, s->stream,
                           n, s->M, s->H, j0, jc, s->cohort.dosage.p, sn.lo.p, sn.hi.p, sn.mask.p, sn.t.p, dose.p);
        for (size_t r = 0; r < runs.size(); ++r)
            scan_lmm_rotate(s, n_ld, runs[r].second - runs[r].first, 1, 1, 1, jc, lm.U.p + (size_t)run_eig[r] * n * n,
                            dose.p + runs[r].first, xs.p + runs[r].first * n_ld);
        GBRS_HIP_CHECK(hipEventRecord(rotate_ring.ev[2 * slot + 1], s->stream));
        GBRS_HIP_CHECK(hipGetLastError());
        for (int64_t p0 = 0; p0 < P; p0 += SC_PCHUNK) {
            const int64_t pc = std::min(SC_PCHUNK, P - p0);
            GBRS_TRY(product_ring.next(&slot));
            GBRS_HIP_CHECK(hipEventRecord(product_ring.ev[2 * slot], s->stream));
            for (size_t r = 0; r < runs.size(); ++r) {
                const int64_t tile0 = runs[r].first / SC_ROWS, tiles = (runs[r].second + SC_ROWS - 1) / SC_ROWS - tile0;
                hipLaunchKernelGGL(lmm_snp_lod_kernel, dim3((unsigned)tiles, (unsigned)((pc + SC_COLS - 1) / SC_COLS)), dim3(SC_THREADS),
                                   LS_LDS_BYTES, s->stream, jc, runs[r].first, runs[r].second, tile0, pc, n_ld, jc, cz, 0.5 * n, xs.p,
                                   cols.p + (size_t)run_eig[r] * (cz + 2) * q_stride + p0 * n_ld, q_stride,
                                   rss_all.p + (size_t)run_eig[r] * P + p0, d_lod.p, d_used.p);
            }
            GBRS_HIP_CHECK(hipEventRecord(product_ring.ev[2 * slot + 1], s->stream));
            hipLaunchKernelGGL(lmm_snp_peak_kernel, dim3((unsigned)nc, (unsigned)pc), dim3(64), 0, s->stream, j0, jc, jc, nc,
                               sn.d_off.p, d_used.p, d_lod.p, d_peak.p + p0 * nc, d_index.p + p0 * nc, d_count.p + p0 * nc);
            GBRS_HIP_CHECK(hipGetLastError());
            if (lod)        // waits for the kernels before it on the stream; the next chunk's product overwrites d_lod after it
                GBRS_HIP_CHECK(hipMemcpy2DAsync(lod + p0 * M_snp + j0, (size_t)M_snp * sizeof(double), d_lod.p,
                                                (size_t)jc * sizeof(double), (size_t)jc * sizeof(double), (size_t)pc,
                                                hipMemcpyDeviceToHost, s->stream));
            if (used)
                GBRS_HIP_CHECK(hipMemcpy2DAsync(used + p0 * M_snp + j0, (size_t)M_snp, d_used.p, (size_t)jc, (size_t)jc, (size_t)pc,
                                                hipMemcpyDeviceToHost, s->stream));
        }
    }
    GBRS_TRY(timed_wait(s));
    GBRS_TRY(null_ring.drain());
    GBRS_TRY(rotate_ring.drain());
    GBRS_TRY(product_ring.drain());
    GBRS_TRY(snp_peaks_out(d_peak, d_index, peak_lod, peak_index));
    GBRS_TRY(copy_out(n_used, d_count, d_count.n));
    gbrs_scan_lmm_snp_info_t &r = s->last.lmm_snp;
    r.P = P;
    r.last_pass_ms = pass_ms(s, r.last_pass_ms);
    r.last_null_ms = null_ring.ms;
    r.last_rotate_ms = rotate_ring.ms;
    r.last_product_ms = product_ring.ms;
    r.column_bytes = cols.bytes() + rss_all.bytes();
    r.peak_device_bytes = s->resident_bytes() + own.bytes;
    return GBRS_OK;
}

int gbrs_scan_lmm_snp_info(gbrs_scan_t *s, gbrs_scan_lmm_snp_info_t *info) {
    if (!s || !info) return fail(GBRS_ERR_INVALID, "bad argument");
    *info = s->last.lmm_snp;
    info->M_snp = s->snp.M;
    info->chunk = SS_CHUNK;
    return GBRS_OK;
}

}  // extern "C"

// ---- interactive covariates ------------------------------------------------------------------------------------

extern "C" {

int gbrs_scan_int_prepare(gbrs_scan_t *s, int c, const double *qz, int k, const double *zint) {
    RoctxRange roctx_range("gbrs_scan_int_prepare");
    if (!s) return fail(GBRS_ERR_INVALID, "handle is NULL");
    if (k < 1) return fail(GBRS_ERR_INVALID, "interactive covariates must be at least 1, got %d", k);
    if (c < 1 || c > SC_MAX_C) return fail(GBRS_ERR_INVALID, "covariate columns must be 1..%d (the intercept included), got %d", SC_MAX_C, c);
    if (!qz || !zint) return fail(GBRS_ERR_INVALID, "qz or zint is NULL");
    const int Hx = s->H - 1;
    if (s->Hp + (int64_t)k * Hx > 64)
        return fail(GBRS_ERR_UNSUPPORTED, "%d interactive covariates of %d founders need %lld rows per grid point, more than 64", k, s->H,
                    (long long)(s->Hp + (int64_t)k * Hx));
    const int columns = Hx * (1 + k), hpi = s->Hp + k * Hx <= 16 ? 16 : s->Hp + k * Hx <= 32 ? 32 : 64;
    if (s->cohort.n <= (int64_t)c + columns)
        return fail(GBRS_ERR_INVALID, "%lld samples are too few for %d covariate columns and %d founders with %d interactive covariates: "
                    "need more than %d", (long long)s->cohort.n, c, s->H, k, c + columns);
    const int n = (int)s->cohort.n;
    for (int64_t q = 0; q < (int64_t)n * c; ++q)
        if (!std::isfinite(qz[q]))
            return fail(GBRS_ERR_INVALID, "covariate basis holds a value that is not finite (sample %lld, column %d)", (long long)(q / c),
                        (int)(q % c));
    for (int64_t q = 0; q < (int64_t)n * k; ++q)
        if (!std::isfinite(zint[q]))
            return fail(GBRS_ERR_INVALID, "interactive covariate %d holds a value that is not finite (sample %lld)", (int)(q % k),
                        (long long)(q / k));
    GBRS_TRY(select_device(s->device));
    gbrs_scan::Inter &in = s->inter;
    in.unprepare();                     // the arguments are good: from here on the preparation is being overwritten
    const int64_t n_ld = padded(n), M = s->M;
    GBRS_TRY(in.qz.alloc((size_t)n * c));
    GBRS_TRY(in.zint.alloc((size_t)n * k));
    GBRS_TRY(in.W.alloc((size_t)M * hpi * n_ld));
    GBRS_TRY(resized(in.d_rank, (size_t)2 * M));
    GBRS_HIP_CHECK(hipMemcpy(in.qz.p, qz, in.qz.bytes(), hipMemcpyHostToDevice));
    GBRS_HIP_CHECK(hipMemcpy(in.zint.p, zint, in.zint.bytes(), hipMemcpyHostToDevice));
    GBRS_TRY(timed_open(s));
    auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3((unsigned)M), dim3(SC_THREADS), 0, s->stream, n, M, s->H, s->Hp, c, k, n_ld, s->cohort.dosage.p,
                           in.qz.p, in.zint.p, in.W.p, in.d_rank.p, in.d_rank.p + M);
    };
    if (hpi == 16) launch(scan_int_prepare_kernel<16>);
    else if (hpi == 32) launch(scan_int_prepare_kernel<32>);
    else launch(scan_int_prepare_kernel<64>);
    GBRS_TRY(timed_wait(s));
    s->last.inter.last_prepare_ms = pass_ms(s, s->last.inter.last_prepare_ms);
    std::vector<int32_t> rank((size_t)2 * M);
    GBRS_TRY(copy_out(rank.data(), in.d_rank, in.d_rank.n));
    in.rank_full.assign(rank.begin(), rank.begin() + M);
    in.rank_add.assign(rank.begin() + M, rank.end());
    in.n_ld = n_ld;
    in.k = k;
    in.hpi = hpi;
    in.c = c;
    return GBRS_OK;
}

int gbrs_scan_int_run(gbrs_scan_t *s, int64_t P, const double *pheno, double *lod_full, double *lod_add, double *lod_int,
                      double *peak_full, int64_t *peak_full_index, double *peak_full_add, double *peak_int, int64_t *peak_int_index) {
    RoctxRange roctx_range("gbrs_scan_int_run");
    if (!s) return fail(GBRS_ERR_INVALID, "handle is NULL");
    if (s->inter.c == 0) return fail(GBRS_ERR_INVALID, "no interactive covariates on the handle: call gbrs_scan_int_prepare first");
    if (P < 1 || !pheno) return fail(GBRS_ERR_INVALID, "bad argument");
    const gbrs_scan::Inter &in = s->inter;
    const int n = (int)s->cohort.n, nc = s->n_chrom;
    GBRS_TRY(check_finite("phenotype", pheno, n, P));
    GBRS_TRY(select_device(s->device));
    const int64_t pc_max = std::min(P, SC_PCHUNK), M = s->M, n_ld = in.n_ld;
    // which of the three LOD rows a chunk needs on the device: an output's own, and those its peaks are taken from
    const bool need_full = lod_full || peak_full || peak_full_index || peak_full_add, need_add = lod_add || peak_full_add,
               need_int = lod_int || peak_int || peak_int_index;
    DevBuf<double> y, yt, rss0, d_full, d_add, d_int, d_peak, d_peak_add;      // the call's own; the pass reports no peak
    DevBuf<int64_t> d_index;
    GBRS_TRY(y.alloc((size_t)n * pc_max));
    GBRS_TRY(yt.alloc((size_t)pc_max * n_ld));
    GBRS_TRY(rss0.alloc((size_t)pc_max));
    if (need_full) GBRS_TRY(d_full.alloc((size_t)pc_max * M));
    if (need_add) GBRS_TRY(d_add.alloc((size_t)pc_max * M));
    if (need_int) GBRS_TRY(d_int.alloc((size_t)pc_max * M));
    GBRS_TRY(d_peak.alloc((size_t)pc_max * nc));
    GBRS_TRY(d_peak_add.alloc((size_t)pc_max * nc));
    GBRS_TRY(d_index.alloc((size_t)pc_max * nc));
    const unsigned row_blocks = (unsigned)((M * in.hpi + SC_ROWS - 1) / SC_ROWS);
    double t_product = 0.0;
    GBRS_TRY(timed_open(s));
    for (int64_t p0 = 0; p0 < P; p0 += SC_PCHUNK) {
        const int64_t pc = std::min(SC_PCHUNK, P - p0);
        const size_t peaks = (size_t)pc * nc, lods = (size_t)pc * M, peak0 = (size_t)p0 * nc, lod0 = (size_t)p0 * M;
        GBRS_TRY(project(s, in.qz, in.c, n_ld, pheno, P, p0, pc, y, yt.p, rss0.p));
        GBRS_HIP_CHECK(hipEventRecord(s->ev[2], s->stream));
        const dim3 grid(row_blocks, (unsigned)((pc + SC_COLS - 1) / SC_COLS));
        auto launch = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, grid, dim3(SC_THREADS), 0, s->stream, M, pc, n_ld, s->Hp, 0.5 * n, in.W.p, yt.p, rss0.p, d_full.p,
                               d_add.p, d_int.p);
        };
        if (in.hpi == 16) launch(scan_int_lod_kernel<16>);
        else if (in.hpi == 32) launch(scan_int_lod_kernel<32>);
        else launch(scan_int_lod_kernel<64>);
        GBRS_HIP_CHECK(hipEventRecord(s->ev[3], s->stream));
        GBRS_HIP_CHECK(hipGetLastError());
        // the full model's peaks, lod_add at them, then the interaction's peaks through the same two tables
        if (need_full) {
            hipLaunchKernelGGL(scan_peak_kernel, dim3((unsigned)nc, (unsigned)pc), dim3(64), 0, s->stream, M, nc, s->d_point_off.p,
                               d_full.p, d_peak.p, d_index.p);
            if (peak_full_add)
                hipLaunchKernelGGL(scan_int_peak_add_kernel, dim3((unsigned)((peaks + 63) / 64)), dim3(64), 0, s->stream, M,
                                   (int64_t)peaks, nc, d_index.p, d_add.p, d_peak_add.p);
            GBRS_HIP_CHECK(hipGetLastError());
            GBRS_HIP_CHECK(hipStreamSynchronize(s->stream));
            GBRS_TRY(copy_out(lod_full, d_full, lods, lod0));
            GBRS_TRY(copy_out(peak_full, d_peak, peaks, peak0));
            GBRS_TRY(copy_out(peak_full_index, d_index, peaks, peak0));
            GBRS_TRY(copy_out(peak_full_add, d_peak_add, peaks, peak0));
        }
        if (need_int) {
            hipLaunchKernelGGL(scan_peak_kernel, dim3((unsigned)nc, (unsigned)pc), dim3(64), 0, s->stream, M, nc, s->d_point_off.p,
                               d_int.p, d_peak.p, d_index.p);
            GBRS_HIP_CHECK(hipGetLastError());
            GBRS_HIP_CHECK(hipStreamSynchronize(s->stream));
            GBRS_TRY(copy_out(lod_int, d_int, lods, lod0));
            GBRS_TRY(copy_out(peak_int, d_peak, peaks, peak0));
            GBRS_TRY(copy_out(peak_int_index, d_index, peaks, peak0));
        }
        GBRS_HIP_CHECK(hipStreamSynchronize(s->stream));
        GBRS_TRY(copy_out(lod_add, d_add, lods, lod0));
        t_product += elapsed_ms(s->ev[2], s->ev[3], 0.0);
    }
    GBRS_TRY(timed_wait(s));
    s->last.inter.last_run_ms = pass_ms(s, s->last.inter.last_run_ms);
    s->last.inter.last_product_ms = t_product;
    return GBRS_OK;
}

int gbrs_scan_int_info(gbrs_scan_t *s, gbrs_scan_int_info_t *info, int32_t *rank_full, int32_t *rank_add) {
    if (!s) return fail(GBRS_ERR_INVALID, "handle is NULL");
    const gbrs_scan::Inter &in = s->inter;
    if (info) {
        *info = s->last.inter;
        info->n = s->cohort.n;
        info->M = s->M;
        info->H = s->H;
        info->c = in.c;
        info->k = in.k;
        info->HPI = in.hpi;
        info->device_bytes = in.c > 0 ? in.bytes() : 0;
    }
    if (rank_full && in.c > 0) std::memcpy(rank_full, in.rank_full.data(), in.rank_full.size() * sizeof(int32_t));
    if (rank_add && in.c > 0) std::memcpy(rank_add, in.rank_add.data(), in.rank_add.size() * sizeof(int32_t));
    return GBRS_OK;
}

}  // extern "C"
