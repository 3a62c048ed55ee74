// The two inputs of `gbrs reconstruct` that the reference makes with `gbrs get-transition-prob` and
// `gbrs get-alignment-spec` (gbrs/gbrs_utils.py:101-187, :208-294, :297-379).
//
//   gbrs_ri_transition_tables   one lane per output double: entry e (0..8) of marker interval j.  The interval's
//                               chromosome comes from a bisection of the chromosomes' first-interval offsets, so an
//                               interval is always the difference of two markers of one chromosome.  Every lane
//                               recomputes R, gamma and log(1 + gamma) of its interval (there is no reuse to win at
//                               nine numbers per interval); consecutive lanes store consecutive doubles.
//   gbrs_alignment_spec         one lane per (gene, strain) row: the row's files are added in file order, divided by
//                               the number of files the strain lists, summed left to right, and scaled by the row's
//                               Euclidean norm.  The S accumulators are statically indexed registers behind a template
//                               on the next power of two (as tensor_hap_sums_kernel, tensor.hip).
//
// Both are plain C++ compiled with -ffp-contract=off: the operation order is the reference's, the adds and the divide of
// the specificity rows are bit-identical to numpy's, and log / sqrt are the device library's (within an ulp of libm's).
// Neither kernel holds an atomic: both are bit-identical from run to run.
#include "common.h"

#include <algorithm>
#include <cmath>

using namespace gbrs;

namespace {

constexpr unsigned HI_BLOCK = 256;
inline unsigned hi_grid(uint64_t n) { return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((n + HI_BLOCK - 1) / HI_BLOCK, 4096)); }

// largest c in [0, n_chroms) with first[c] <= j   (first non-decreasing, first[0] = 0 <= j < first[n_chroms]): the
// chromosome that owns interval j; chromosomes without an interval share their offset with the next one and are skipped
__device__ __forceinline__ int64_t interval_chromosome(const int64_t *__restrict__ first, int64_t n_chroms, int64_t j) {
    int64_t lo = 0, hi = n_chroms - 1;
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo + 1) >> 1);
        if (first[mid] <= j) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// ris_step (gbrs_utils.py:101-187), forward direction: out[j][to][from] in the reference's [dt1id, dt2id] order
__global__ void __launch_bounds__(HI_BLOCK)
ri_transition_kernel(int64_t n_intervals, int64_t n_chroms, const double *__restrict__ cm,
                     const int64_t *__restrict__ chrom_ptr, const int64_t *__restrict__ first_interval,
                     const uint8_t *__restrict__ is_x, double gamma_scale, double epsilon, double *__restrict__ out) {
    const uint64_t total = (uint64_t)n_intervals * 9;
    for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < total; k += (uint64_t)gridDim.x * blockDim.x) {
        const int64_t j = (int64_t)(k / 9);
        const int e = (int)(k - (uint64_t)j * 9);
        double v;
        if (e >= 3 && e < 6) {
            v = log(1 / 3.0);
        } else {
            const int64_t c = interval_chromosome(first_interval, n_chroms, j);
            const int64_t m = chrom_ptr[c] + (j - first_interval[c]);       // m + 1 < chrom_ptr[c + 1]
            double r = cm[m + 1] - cm[m];
            if (r < epsilon) r = epsilon;
            const bool x = is_x[c] != 0;
            const double R = x ? (2 * r) / (1.0 + 4.0 * r) : 4.0 * r / (1 + 6.0 * r);
            const double g = R * gamma_scale;
            const double z = log(1 + g);
            const double stay = 1.0 - R, move = R;                        // row 0, and row 2 of an autosome mirrored
            const double stay2 = x ? 1.0 - 2.0 * R : 1.0 - R, move2 = x ? 2.0 * R : R;
            double a;
            switch (e) {
            case 0: a = stay; break;
            case 2: a = move; break;
            case 6: a = move2; break;
            case 8: a = stay2; break;
            default: a = g; break;                                         // 1 and 7: into the heterozygote
            }
            v = log(a) - z;
        }
        out[k] = v;
    }
}

// tables [F][G][S]; row = g * S + i is strain i of gene g.  axes (G x S x S), ases (G x S), avecs (G x S x S); has_avec
// (G, zeroed by the caller) receives 1 from every row whose sum exceeds min_expr.
template <int ST>
__global__ void __launch_bounds__(HI_BLOCK)
alignment_spec_kernel(int64_t n_genes, int n_strains, const double *__restrict__ tables,
                      const int64_t *__restrict__ strain_ptr, const int64_t *__restrict__ strain_div, double min_expr,
                      double *__restrict__ axes, double *__restrict__ ases, double *__restrict__ avecs,
                      uint8_t *__restrict__ has_avec) {
    const uint64_t rows = (uint64_t)n_genes * n_strains;
    for (uint64_t row = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; row < rows; row += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t g = row / n_strains;
        const int i = (int)(row - g * n_strains);
        double acc[ST];
#pragma unroll
        for (int t = 0; t < ST; ++t) acc[t] = 0.0;
        for (int64_t f = strain_ptr[i]; f < strain_ptr[i + 1]; ++f) {
            const double *src = tables + ((uint64_t)f * n_genes + g) * n_strains;
#pragma unroll
            for (int t = 0; t < ST; ++t)
                if (t < n_strains) acc[t] += src[t];
        }
        const double div = (double)strain_div[i];
        double sum = 0.0, sq = 0.0;
#pragma unroll
        for (int t = 0; t < ST; ++t)
            if (t < n_strains) {
                acc[t] /= div;
                sum += acc[t];
                sq += acc[t] * acc[t];
            }
        const bool scale = sum > 1e-6;                                     // unit_vector (gbrs_utils.py:63-67)
        const double norm = sqrt(sq);
#pragma unroll
        for (int t = 0; t < ST; ++t)
            if (t < n_strains) {
                axes[row * n_strains + t] = acc[t];
                avecs[row * n_strains + t] = scale ? acc[t] / norm : acc[t];
            }
        ases[row] = sum;
        if (sum > min_expr) has_avec[g] = 1;
    }
}

template <int ST>
void launch_alignment_spec(int64_t n_genes, int n_strains, const double *tables, const int64_t *strain_ptr,
                           const int64_t *strain_div, double min_expr, double *axes, double *ases, double *avecs,
                           uint8_t *has_avec) {
    hipLaunchKernelGGL((alignment_spec_kernel<ST>), dim3(hi_grid((uint64_t)n_genes * n_strains)), dim3(HI_BLOCK), 0, nullptr,
                       n_genes, n_strains, tables, strain_ptr, strain_div, min_expr, axes, ases, avecs, has_avec);
}

}  // namespace

extern "C" {

int gbrs_ri_transition_tables(const double *cm, const int64_t *chrom_ptr, const uint8_t *is_x, int64_t num_chroms,
                              double gamma_scale, double epsilon, int device, double *out) {
    RoctxRange roctx_range("gbrs_ri_transition_tables");
    if (num_chroms < 0) return fail(GBRS_ERR_INVALID, "num_chroms is negative");
    if (!chrom_ptr) return fail(GBRS_ERR_INVALID, "chrom_ptr is NULL");
    if (num_chroms > 0 && !is_x) return fail(GBRS_ERR_INVALID, "is_x is NULL");
    if (chrom_ptr[0] != 0) return fail(GBRS_ERR_INVALID, "chrom_ptr must start at 0");
    std::vector<int64_t> first((size_t)num_chroms + 1, 0);
    for (int64_t c = 0; c < num_chroms; ++c) {
        const int64_t n = chrom_ptr[c + 1] - chrom_ptr[c];
        if (n < 0) return fail(GBRS_ERR_INVALID, "chrom_ptr decreases at chromosome %lld", (long long)c);
        first[c + 1] = first[c] + std::max<int64_t>(n - 1, 0);
    }
    const int64_t n_markers = chrom_ptr[num_chroms], n_intervals = first[num_chroms];
    if (n_markers > 0 && !cm) return fail(GBRS_ERR_INVALID, "cm is NULL");
    if (n_intervals == 0) return GBRS_OK;
    if (!out) return fail(GBRS_ERR_INVALID, "out is NULL");
    GBRS_TRY(select_device(device));
    DevBuf<double> d_cm, d_out;
    DevBuf<int64_t> d_ptr, d_first;
    DevBuf<uint8_t> d_x;
    GBRS_TRY(d_cm.alloc(n_markers));
    GBRS_TRY(d_ptr.alloc(num_chroms + 1));
    GBRS_TRY(d_first.alloc(num_chroms + 1));
    GBRS_TRY(d_x.alloc(num_chroms));
    GBRS_TRY(d_out.alloc((size_t)n_intervals * 9));
    GBRS_HIP_CHECK(hipMemcpy(d_cm.p, cm, d_cm.bytes(), hipMemcpyHostToDevice));
    GBRS_HIP_CHECK(hipMemcpy(d_ptr.p, chrom_ptr, d_ptr.bytes(), hipMemcpyHostToDevice));
    GBRS_HIP_CHECK(hipMemcpy(d_first.p, first.data(), d_first.bytes(), hipMemcpyHostToDevice));
    GBRS_HIP_CHECK(hipMemcpy(d_x.p, is_x, d_x.bytes(), hipMemcpyHostToDevice));
    hipLaunchKernelGGL(ri_transition_kernel, dim3(hi_grid((uint64_t)n_intervals * 9)), dim3(HI_BLOCK), 0, nullptr,
                       n_intervals, num_chroms, d_cm.p, d_ptr.p, d_first.p, d_x.p, gamma_scale, epsilon, d_out.p);
    GBRS_HIP_CHECK(hipGetLastError());
    GBRS_HIP_CHECK(hipMemcpy(out, d_out.p, d_out.bytes(), hipMemcpyDeviceToHost));
    return GBRS_OK;
}

int gbrs_alignment_spec(const double *tables, const int64_t *strain_ptr, const int64_t *strain_div, int64_t num_genes,
                        int num_strains, double min_expr, int device, double *axes, double *ases, double *avecs,
                        uint8_t *has_avec) {
    RoctxRange roctx_range("gbrs_alignment_spec");
    if (num_strains < 1 || num_strains > 32)
        return fail(GBRS_ERR_UNSUPPORTED, "%d parental strains: 1 to 32 are supported", num_strains);
    if (num_genes < 0) return fail(GBRS_ERR_INVALID, "num_genes is negative");
    if (!strain_ptr || !strain_div) return fail(GBRS_ERR_INVALID, "strain_ptr / strain_div is NULL");
    if (strain_ptr[0] != 0) return fail(GBRS_ERR_INVALID, "strain_ptr must start at 0");
    for (int i = 0; i < num_strains; ++i) {
        if (strain_ptr[i + 1] < strain_ptr[i]) return fail(GBRS_ERR_INVALID, "strain_ptr decreases at strain %d", i);
        if (strain_div[i] < 1 || strain_div[i] < strain_ptr[i + 1] - strain_ptr[i])
            return fail(GBRS_ERR_INVALID, "strain %d: %lld listed files for %lld tables", i, (long long)strain_div[i],
                        (long long)(strain_ptr[i + 1] - strain_ptr[i]));
    }
    const int64_t n_files = strain_ptr[num_strains];
    if (num_genes == 0) return GBRS_OK;
    if ((n_files > 0 && !tables) || !axes || !ases || !avecs || !has_avec)
        return fail(GBRS_ERR_INVALID, "tables / axes / ases / avecs / has_avec is NULL");
    GBRS_TRY(select_device(device));
    const size_t S = (size_t)num_strains, G = (size_t)num_genes;
    DevBuf<double> d_tab, d_axes, d_ases, d_avecs;
    DevBuf<int64_t> d_ptr, d_div;
    DevBuf<uint8_t> d_has;
    GBRS_TRY(d_tab.alloc((size_t)n_files * G * S));
    GBRS_TRY(d_axes.alloc(G * S * S));
    GBRS_TRY(d_ases.alloc(G * S));
    GBRS_TRY(d_avecs.alloc(G * S * S));
    GBRS_TRY(d_ptr.alloc(S + 1));
    GBRS_TRY(d_div.alloc(S));
    GBRS_TRY(d_has.alloc(G));
    if (n_files > 0) GBRS_HIP_CHECK(hipMemcpy(d_tab.p, tables, d_tab.bytes(), hipMemcpyHostToDevice));
    GBRS_HIP_CHECK(hipMemcpy(d_ptr.p, strain_ptr, d_ptr.bytes(), hipMemcpyHostToDevice));
    GBRS_HIP_CHECK(hipMemcpy(d_div.p, strain_div, d_div.bytes(), hipMemcpyHostToDevice));
    GBRS_HIP_CHECK(hipMemset(d_has.p, 0, d_has.bytes()));
#define GBRS_LAUNCH_SPEC(ST)                                                                                         \
    launch_alignment_spec<ST>(num_genes, num_strains, d_tab.p, d_ptr.p, d_div.p, min_expr, d_axes.p, d_ases.p,        \
                              d_avecs.p, d_has.p)
    if (num_strains <= 1) GBRS_LAUNCH_SPEC(1);
    else if (num_strains <= 2) GBRS_LAUNCH_SPEC(2);
    else if (num_strains <= 4) GBRS_LAUNCH_SPEC(4);
    else if (num_strains <= 8) GBRS_LAUNCH_SPEC(8);
    else if (num_strains <= 16) GBRS_LAUNCH_SPEC(16);
    else GBRS_LAUNCH_SPEC(32);
#undef GBRS_LAUNCH_SPEC
    GBRS_HIP_CHECK(hipGetLastError());
    GBRS_HIP_CHECK(hipMemcpy(axes, d_axes.p, d_axes.bytes(), hipMemcpyDeviceToHost));
    GBRS_HIP_CHECK(hipMemcpy(ases, d_ases.p, d_ases.bytes(), hipMemcpyDeviceToHost));
    GBRS_HIP_CHECK(hipMemcpy(avecs, d_avecs.p, d_avecs.bytes(), hipMemcpyDeviceToHost));
    GBRS_HIP_CHECK(hipMemcpy(has_avec, d_has.p, d_has.bytes(), hipMemcpyDeviceToHost));
    return GBRS_OK;
}

}  // extern "C"
