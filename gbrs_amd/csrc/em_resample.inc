// Bootstrap replicates (GBRS_EM_RESAMPLE, gbrs_em_resample, gbrs_em_bootstrap_*; DESIGN.md §19).  Included by em.hip
// inside namespace gbrs.
//
// Replicate b gives file row r the weight  w(b, r) = sum_{k < c_r} P(u(b, r, k)),  c_r the row's base count (1 without a
// count vector), u(b, r, k) word k mod 4 of Philox4x32-10 with counter (r lo, r hi, k div 4, b) and key (seed lo, seed hi),
// P(u) = #{j : u >= T[j]} with T[j] = floor(2^32 * sum_{i <= j} e^-1 / i!): a Poisson(1) deviate by inversion on integers,
// so w is Poisson(c_r) up to the 2^-32 grain of the table, an integer, and a function of (seed, b, r, c_r) alone - however
// the c_r draws of a row are split over lanes, the same numbers are added.

#include "philox.h"      // philox4x32_10, shared with hmm_sample.inc

// P(u): how many of the 13 thresholds u reaches
__device__ __forceinline__ uint32_t poisson1_by_inversion(uint32_t u) {
    uint32_t n = 0;
    n += u >= 1580030168u; n += u >= 3160060337u; n += u >= 3950075421u; n += u >= 4213413783u;
    n += u >= 4279248373u; n += u >= 4292415291u; n += u >= 4294609777u; n += u >= 4294923276u;
    n += u >= 4294962463u; n += u >= 4294966817u; n += u >= 4294967252u; n += u >= 4294967292u;
    n += u >= 4294967295u;
    return n;
}

// the draws 4 k4 .. 4 k4 + 3 of row r that lie below c
__device__ __forceinline__ uint32_t resample_block(uint64_t r, uint32_t k4, uint32_t c, uint32_t b, uint32_t k0, uint32_t k1) {
    uint32_t ctr[4] = {(uint32_t)r, (uint32_t)(r >> 32), k4, b};
    philox4x32_10(ctr, k0, k1);
    const uint32_t left = c - 4u * k4;         // >= 1
    uint32_t w = poisson1_by_inversion(ctr[0]);
    if (left > 1) w += poisson1_by_inversion(ctr[1]);
    if (left > 2) w += poisson1_by_inversion(ctr[2]);
    if (left > 3) w += poisson1_by_inversion(ctr[3]);
    return w;
}

// base count as integers; anything negative, fractional, not finite or >= 2^32 raises *bad
__global__ void __launch_bounds__(256)
resample_base_kernel(uint64_t R, const double *__restrict__ count, uint32_t *__restrict__ base, int *__restrict__ bad) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= R) return;
    const double c = count[r];
    if (!(c >= 0.0 && c < 4294967296.0) || c != floor(c)) { *bad = 1; base[r] = 0; return; }
    base[r] = (uint32_t)c;
}

// rows whose count is above the cut get a workgroup each (resample_big_kernel); list == nullptr: count them only
__global__ void __launch_bounds__(256)
resample_big_rows_kernel(uint64_t R, const uint32_t *__restrict__ base, uint32_t cut, uint32_t *__restrict__ counter,
                         uint32_t *__restrict__ list) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= R || base[r] <= cut) return;
    const uint32_t i = atomicAdd(counter, 1u);
    if (list) list[i] = (uint32_t)r;
}

// one lane per row.  RESTORE: the base weights themselves
template <bool RESTORE>
__global__ void __launch_bounds__(256)
resample_draw_kernel(uint64_t R, const uint32_t *__restrict__ base, uint32_t cut, uint32_t b, uint32_t k0, uint32_t k1,
                     double *__restrict__ weight) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= R) return;
    const uint32_t c = base ? base[r] : 1u;
    if (RESTORE) { weight[r] = (double)c; return; }
    if (c > cut) return;                       // resample_big_kernel writes it
    uint64_t w = 0;
    for (uint32_t k4 = 0; 4ull * k4 < c; ++k4) w += resample_block(r, k4, c, b, k0, k1);
    weight[r] = (double)w;
}

// one workgroup per row above the cut: thread t takes the Philox blocks t, t + 256, ...; integer sums, any order
__global__ void __launch_bounds__(256)
resample_big_kernel(uint32_t n_big, const uint32_t *__restrict__ big_rows, const uint32_t *__restrict__ base, uint32_t b,
                    uint32_t k0, uint32_t k1, double *__restrict__ weight) {
    __shared__ unsigned long long part[4];
    if (blockIdx.x >= n_big) return;
    const uint64_t r = big_rows[blockIdx.x];
    const uint32_t c = base[r];
    const uint32_t n_blocks = (uint32_t)(((uint64_t)c + 3) >> 2);
    unsigned long long w = 0;
    for (uint32_t k4 = threadIdx.x; k4 < n_blocks; k4 += 256) w += resample_block(r, k4, c, b, k0, k1);
    for (int off = 32; off > 0; off >>= 1) w += __shfl_down(w, off, WAVE);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = w;
    __syncthreads();
    if (threadIdx.x == 0) weight[r] = (double)(part[0] + part[1] + part[2] + part[3]);
}

// the row weights onto the words of the tiles and onto the long rows (TileLayout::word_row / long_row)
__global__ void __launch_bounds__(256)
install_weights_kernel(uint64_t n, const uint32_t *__restrict__ row_of, const double *__restrict__ weight,
                       double *__restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t r = row_of[i];
    out[i] = r == 0xFFFFFFFFu ? 0.0 : weight[r];
}

// ---- replicate statistics --------------------------------------------------------------------------------------------
// sum of n doubles on one workgroup: thread t adds the elements t, t + 1024, ... in order, then a fixed tree - the same
// bits on every launch
__global__ void __launch_bounds__(1024)
stats_sum_kernel(uint64_t n, const double *__restrict__ v, double *__restrict__ out) {
    __shared__ double s[1024];
    double a = 0.0;
    for (uint64_t i = threadIdx.x; i < n; i += 1024) a += v[i];
    s[threadIdx.x] = a;
    __syncthreads();
    for (int half = 512; half > 0; half >>= 1) {
        if ((int)threadIdx.x < half) s[threadIdx.x] += s[threadIdx.x + half];
        __syncthreads();
    }
    if (threadIdx.x == 0) *out = s[0];
}

// this replicate's TPM = theta * (1e6 / sum theta) and expected counts, locus-major -> (H x L)
__global__ void __launch_bounds__(256)
stats_current_kernel(uint32_t L, uint32_t H, const double *__restrict__ theta, const double *__restrict__ counts,
                     const double *__restrict__ theta_sum, double *__restrict__ cur_tpm, double *__restrict__ cur_cnt) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (uint64_t)L * H) return;
    const uint32_t l = (uint32_t)(i / H), h = (uint32_t)(i - (uint64_t)l * H);
    const double scale = 1000000.0 / *theta_sum;
    cur_tpm[(size_t)h * L + l] = theta[i] * scale;
    cur_cnt[(size_t)h * L + l] = counts[i];
}

// gene level: out (H x G) = the members' values added in member order (as gbrs_em_group_sums)
__global__ void __launch_bounds__(256)
stats_group_kernel(uint32_t L, uint32_t H, int64_t G, const int64_t *__restrict__ gptr, const int64_t *__restrict__ members,
                   const double *__restrict__ cur, double *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= G * (int64_t)H) return;
    const int64_t h = i / G, g = i - h * G;
    double s = 0.0;
    for (int64_t k = gptr[g]; k < gptr[g + 1]; ++k) s += cur[(size_t)h * L + members[k]];
    out[i] = s;
}

// Welford update with the values of replicate number nrep (1-based): one thread per column j of the (H x n) matrix, its H
// elements and then their total (added in haplotype order)
__global__ void __launch_bounds__(256)
stats_fold_kernel(uint64_t n, uint32_t H, uint32_t nrep, const double *__restrict__ cur, double *__restrict__ mean,
                  double *__restrict__ m2, double *__restrict__ tot_mean, double *__restrict__ tot_m2) {
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const double k = (double)nrep;
    double tot = 0.0;
    for (uint32_t h = 0; h < H; ++h) {
        const size_t i = (size_t)h * n + j;
        const double x = cur[i], m0 = nrep == 1 ? 0.0 : mean[i], d = x - m0, m1 = m0 + d / k;
        mean[i] = m1;
        m2[i] = (nrep == 1 ? 0.0 : m2[i]) + d * (x - m1);
        tot += x;
    }
    const double m0 = nrep == 1 ? 0.0 : tot_mean[j], d = tot - m0, m1 = m0 + d / k;
    tot_mean[j] = m1;
    tot_m2[j] = (nrep == 1 ? 0.0 : tot_m2[j]) + d * (tot - m1);
}
