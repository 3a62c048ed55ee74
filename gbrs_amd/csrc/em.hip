// EMASE Model-4 EM on MI355X (gfx950).  See include/gbrs_hip.h for the boundary and DESIGN.md
// for the data layout and kernel inventory.
//
// One EM step of the reference (emase/EMfactory.py:214-232 with the Model-4 branch :204-208)
// never needs the per-entry posterior: with
//       den[r]  = sum_{(h,l) in row r} theta[h,l]                         (normalize_reads READ)
//       A[h,l]  = sum_{r in column (h,l)} count[r] / den[r]               (sum READ)
// the update is theta'[h,l] = theta[h,l] * A[h,l] / eff_len[h,l], and the expected read counts
// of that E-step are theta[h,l] * A[h,l].  Everything below computes den and A.
#include "common.h"
#include "em_layout.h"
#include "em_step.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdlib>

namespace gbrs {

// ------------------------------------------------------------------------------------------
// Small per-iteration kernels (M-step, convergence), shared by every E-step layout.
// theta, acc, counts, eff_len are locus-major on the device: index l*H + h, so one locus is one
// 64-byte line at H = 8.
// ------------------------------------------------------------------------------------------

struct EmScalars {          // lives in device memory, one per handle
    double s_prev, s_new;   // sum of theta over everything before / after the step
    double err_sum;         // total TPM change of the last step
    double pc_before, pc_after;
    int stop;               // set once err_sum <= target (EMfactory.py:267)
    int iters_done;         // EM steps applied to theta
    int float_error;        // a referenced row had den == 0 (FloatingPointError in the reference)
    int ticket;             // arrival counter of err_finish_kernel (reset by its last block)
};

constexpr int RED_BLOCKS = 256;   // partial slots of the two-level deterministic reductions
constexpr int RED_THREADS = 256;

// theta' = theta * A / len, counts = theta * A, per-locus totals before and after, block partials.
// mode 0: EM step.  mode 1: prepare (theta treated as 1 everywhere).
template <int MODE>
__global__ void __launch_bounds__(RED_THREADS)
mstep_kernel(uint32_t L, uint32_t H, double *__restrict__ theta, const double *__restrict__ acc,
             const double *__restrict__ eff_len, double *__restrict__ counts,
             double *__restrict__ tot_prev, double *__restrict__ tot_new,
             double *__restrict__ msums, uint32_t cap, const EmScalars *__restrict__ sc) {
    __shared__ double lds[16];
    if (MODE == 0 && sc->stop) return;
    double p_prev = 0.0, p_new = 0.0;
    for (uint32_t l = blockIdx.x * blockDim.x + threadIdx.x; l < L; l += gridDim.x * blockDim.x) {
        double tp = 0.0, tn = 0.0;
        const size_t base = (size_t)l * H;
        for (uint32_t h = 0; h < H; ++h) {
            const double t = MODE == 0 ? theta[base + h] : 1.0;
            const double c = t * acc[base + h];
            double tnew = c;
            if (eff_len) tnew = c / eff_len[base + h];
            counts[base + h] = c;
            theta[base + h] = tnew;
            tp += t;
            tn += tnew;
        }
        tot_prev[l] = tp;
        tot_new[l] = tn;
        p_prev += tp;
        p_new += tn;
    }
    double a = block_sum(p_prev, lds);
    double b = block_sum(p_new, lds);
    if (threadIdx.x == 0) {
        msums[blockIdx.x] = a;
        msums[cap + blockIdx.x] = b;
    }
}

__device__ __forceinline__ double reduce_partials(const double *__restrict__ p, int n, double *lds) {
    double v = 0.0;
    for (int i = threadIdx.x; i < n; i += blockDim.x) v += p[i];
    return block_sum(v, lds);
}

#include "em_mstep.inc"      // mstep_elem_kernel<MODE, H>, mstep_gather_kernel<H, EXTRA, LEN>: H a power of two

constexpr int ERR_BLOCKS = 64;
// err_sum = sum_l | tot_new[l]*1e6/S_new - tot_prev[l]*1e6/S_prev |  (EMfactory.py:268-278), then the
// bookkeeping of the step (err history, iteration counter, stop flag; :266-267).  Every block
// reduces the M-step's block partials to S_prev / S_new itself (fixed order), writes its partial
// of err_sum and takes a ticket; the block that draws the last ticket sums the partials in fixed
// order, so the result does not depend on the order in which blocks finish.
// Arguments of the error pass, as one value: gather_kernel carries them for the deferred form.
struct ErrArgs {
    uint32_t L;
    int nblocks;                 // workgroups of the M-step launch = block sums to add up
    uint32_t cap;                // offset of the second block-sum array / of the error partials (x2)
    const double *tot_prev, *tot_new;
    double *partials;
    EmScalars *sc;
    double target_err;
    double *err_hist;
    int err_hist_cap;
    uint32_t n_err_blocks;       // workgroups that run the pass (0: none)
};

__device__ __forceinline__ void err_finish_body(const ErrArgs &ea, unsigned bid) {
    const uint32_t L = ea.L;
    const int nblocks = ea.nblocks;
    const double *__restrict__ tot_prev = ea.tot_prev, *__restrict__ tot_new = ea.tot_new;
    double *__restrict__ partials = ea.partials;
    EmScalars *__restrict__ sc = ea.sc;
    const double target_err = ea.target_err;
    double *__restrict__ err_hist = ea.err_hist;
    const int err_hist_cap = ea.err_hist_cap;
    const unsigned nb = ea.n_err_blocks;
    __shared__ double lds[16];
    __shared__ double s_sums[2];
    __shared__ int s_last;
    // (one read of the flag per workgroup: a partner handle's pair_err_kernel may raise it while this pass is running)
    if (threadIdx.x == 0) s_last = sc->stop;
    __syncthreads();
    if (s_last) return;
    __syncthreads();                                            // s_last is written again below
    double a = reduce_partials(partials, nblocks, lds);
    double b = reduce_partials(partials + ea.cap, nblocks, lds);
    if (threadIdx.x == 0) {
        s_sums[0] = a;
        s_sums[1] = b;
    }
    __syncthreads();
    const double cp = 1000000.0 / s_sums[0], cn = 1000000.0 / s_sums[1];
    double e = 0.0;
    for (uint32_t l = bid * blockDim.x + threadIdx.x; l < L; l += nb * blockDim.x)
        e += fabs(tot_new[l] * cn - tot_prev[l] * cp);
    e = block_sum(e, lds);
    if (threadIdx.x == 0) {
        partials[2 * (size_t)ea.cap + bid] = e;
        __threadfence();                                        // publish before the ticket
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");          // (the compiler may drop the fence's own wait)
        const int ticket = atomicAdd(&sc->ticket, 1);
        s_last = ticket == (int)nb - 1;
        if (s_last) __threadfence();                            // acquire the other blocks' partials
    }
    __syncthreads();
    if (!s_last) return;
    double tot = 0.0;
    for (int i = threadIdx.x; i < (int)nb; i += blockDim.x)
        tot += __hip_atomic_load(&partials[2 * (size_t)ea.cap + i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    tot = block_sum(tot, lds);
    if (threadIdx.x == 0) {
        sc->ticket = 0;
        sc->s_prev = s_sums[0];
        sc->s_new = s_sums[1];
        sc->err_sum = tot;
        const int it = sc->iters_done;
        if (err_hist && it < err_hist_cap) err_hist[it] = tot;
        sc->iters_done = it + 1;
        if (!(tot > target_err)) sc->stop = 1;
        if (!(s_sums[0] > 0.0) || !(s_sums[1] > 0.0) || tot != tot) sc->float_error = 1;
    }
}

__global__ void __launch_bounds__(RED_THREADS)
err_finish_kernel(ErrArgs ea) {
    err_finish_body(ea, blockIdx.x);
}

// The stopping rule of EMfactory.run (EMfactory.py:266-278) over TWO handles that hold the two locus ranges of one
// sample (gbrs_amd/dist.py PipelinedShardedEM): err_sum = sum over the loci of both ranges of
// | tot_new * 1e6 / S_new - tot_prev * 1e6 / S_prev | with S the totals over both.  One workgroup; when the sum is at or
// under the target it raises both handles' stop flags, so that every later kernel of either handle is a no-op and theta
// stays the stopping iteration's.
struct PairSide {
    uint32_t L;
    int nblocks;
    uint32_t cap;
    const double *tot_prev, *tot_new, *msums;
    EmScalars *sc;
};
struct PairState { int iters, stop; double err; };
__global__ void __launch_bounds__(1024)
pair_err_kernel(PairSide a, PairSide b, double target_err, PairState *__restrict__ ps, double *__restrict__ hist,
                int hist_cap) {
    __shared__ double lds[16];
    __shared__ double s_sum[2];
    if (ps->stop) return;
    double sp = 0.0, sn = 0.0;
    for (int i = threadIdx.x; i < a.nblocks; i += blockDim.x) { sp += a.msums[i]; sn += a.msums[a.cap + i]; }
    for (int i = threadIdx.x; i < b.nblocks; i += blockDim.x) { sp += b.msums[i]; sn += b.msums[b.cap + i]; }
    sp = block_sum(sp, lds);
    sn = block_sum(sn, lds);
    if (threadIdx.x == 0) { s_sum[0] = sp; s_sum[1] = sn; }
    __syncthreads();
    const double cp = 1000000.0 / s_sum[0], cn = 1000000.0 / s_sum[1];
    double e = 0.0;
    for (uint32_t l = threadIdx.x; l < a.L; l += blockDim.x) e += fabs(a.tot_new[l] * cn - a.tot_prev[l] * cp);
    for (uint32_t l = threadIdx.x; l < b.L; l += blockDim.x) e += fabs(b.tot_new[l] * cn - b.tot_prev[l] * cp);
    e = block_sum(e, lds);
    if (threadIdx.x == 0) {
        const int it = ps->iters;
        if (hist && it < hist_cap) hist[it] = e;
        ps->iters = it + 1;
        ps->err = e;
        if (!(e > target_err)) {
            ps->stop = 1;
            a.sc->stop = 1;
            b.sc->stop = 1;
        }
        if (!(s_sum[0] > 0.0) || !(s_sum[1] > 0.0) || e != e) a.sc->float_error = 1;
    }
}

// pseudocount rule, EMfactory.py:105-111: every haplotype of a locus with any nonzero haplotype
// gets +pc, then the whole matrix is rescaled to its previous total.
__global__ void __launch_bounds__(RED_THREADS)
pseudo_add_kernel(uint32_t L, uint32_t H, double pc, double *__restrict__ theta,
                  double *__restrict__ partials) {
    __shared__ double lds[16];
    double before = 0.0, after = 0.0;
    for (uint32_t l = blockIdx.x * blockDim.x + threadIdx.x; l < L; l += gridDim.x * blockDim.x) {
        const size_t base = (size_t)l * H;
        bool any = false;
        double s = 0.0;
        for (uint32_t h = 0; h < H; ++h) {
            const double t = theta[base + h];
            any |= (t != 0.0);
            s += t;
        }
        before += s;
        if (any) {
            double s2 = 0.0;
            for (uint32_t h = 0; h < H; ++h) {
                const double t = theta[base + h] + pc;
                theta[base + h] = t;
                s2 += t;
            }
            after += s2;
        } else {
            after += s;
        }
    }
    double a = block_sum(before, lds);
    double b = block_sum(after, lds);
    if (threadIdx.x == 0) {
        partials[blockIdx.x] = a;
        partials[RED_BLOCKS + blockIdx.x] = b;
    }
}

__global__ void __launch_bounds__(RED_THREADS)
pseudo_scale_kernel(uint64_t n, int nblocks, double *__restrict__ theta,
                    const double *__restrict__ partials, EmScalars *__restrict__ sc) {
    __shared__ double lds[16];
    __shared__ double s_f;
    double a = reduce_partials(partials, nblocks, lds);
    double b = reduce_partials(partials + RED_BLOCKS, nblocks, lds);
    if (threadIdx.x == 0) {
        // (a handle without entries: no locus got the pseudocount, every element is 0 and stays 0 - the reference's
        // 0 / 0 hands back NaN under a numpy warning)
        s_f = b != 0.0 ? a / b : 1.0;
        if (blockIdx.x == 0) {
            sc->pc_before = a;
            sc->pc_after = b;
        }
    }
    __syncthreads();
    const double f = s_f;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += (uint64_t)gridDim.x * blockDim.x)
        theta[i] *= f;
}

// (H x L) row-major host order <-> (L x H) locus-major device order
__global__ void transpose_hl_to_lh(uint32_t L, uint32_t H, const double *__restrict__ src,
                                   double *__restrict__ dst) {
    const uint64_t n = (uint64_t)L * H;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t l = i / H, h = i % H;
        dst[i] = src[(uint64_t)h * L + l];
    }
}
__global__ void transpose_lh_to_hl(uint32_t L, uint32_t H, const double *__restrict__ src,
                                   double *__restrict__ dst) {
    const uint64_t n = (uint64_t)L * H;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t h = i / L, l = i % L;
        dst[i] = src[(uint64_t)l * H + h];
    }
}

// Gene-level segmented sum (EMfactory.py:140-142): out[h][g] = sum over member loci in ascending
// order -- the accumulation order of scipy's csc right-multiplication, so given the same theta
// the result is the reference's bit for bit.  One thread per (gene, haplotype).
__global__ void group_sum_kernel(uint32_t H, int64_t G, const int64_t *__restrict__ gptr,
                                 const int64_t *__restrict__ members,
                                 const double *__restrict__ src_lh, double *__restrict__ out_hg) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= G * (int64_t)H) return;
    const int64_t g = i / H;
    const uint32_t h = i % H;
    double s = 0.0;
    for (int64_t k = gptr[g]; k < gptr[g + 1]; ++k) s += src_lh[(size_t)members[k] * H + h];
    out_hg[(size_t)h * G + g] = s;
}

// ------------------------------------------------------------------------------------------
// E-step, layout 0 ("csc-direct"): works straight on the reference's CSC arrays.  Two passes
// with global float64 atomics; kept as the simple correct baseline and as the cross-check for
// the tiled layout.
// ------------------------------------------------------------------------------------------

template <bool ONES>
__global__ void __launch_bounds__(256)
csc_den_kernel(uint64_t n, uint32_t ncols, uint32_t L, uint32_t H,
               const uint64_t *__restrict__ col_ptr, const uint32_t *__restrict__ ent_row,
               const double *__restrict__ theta, double *__restrict__ den,
               const EmScalars *__restrict__ sc) {
    if (!ONES && sc->stop) return;
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k - (threadIdx.x & 63) >= n) return;
    const bool live = k < n;
    const uint32_t c = entry_column(col_ptr, ncols, live ? k : n - 1, n);
    if (!live) return;
    const uint32_t h = c / L, l = c - h * L;
    const double t = ONES ? 1.0 : theta[(size_t)l * H + h];
    atomicAdd(&den[ent_row[k]], t);
}

template <bool ONES>
__global__ void __launch_bounds__(256)
csc_acc_kernel(uint64_t n, uint32_t ncols, uint32_t L, uint32_t H,
               const uint64_t *__restrict__ col_ptr, const uint32_t *__restrict__ ent_row,
               const double *__restrict__ count, const double *__restrict__ den,
               double *__restrict__ acc, EmScalars *__restrict__ sc, uint32_t relax_zero_weight) {
    if (!ONES && sc->stop) return;
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k - (threadIdx.x & 63) >= n) return;
    const bool live = k < n;
    const uint32_t c = entry_column(col_ptr, ncols, live ? k : n - 1, n);
    double w = 0.0;
    if (live) {
        const uint32_t r = ent_row[k];
        const double d = den[r];
        const double cnt = count ? count[r] : 1.0;
        // (resampling handles: a zero-weight row takes no part, its own zero denominator is no float error)
        if (d > 0.0) w = cnt / d; else if (!(relax_zero_weight && cnt == 0.0)) sc->float_error = 1;
    }
    const uint32_t c0 = __shfl(c, 0, WAVE);
    if (__all(c == c0)) {
        w = wave_sum(w);
        if ((threadIdx.x & 63) == 0) {
            const uint32_t h = c0 / L, l = c0 - h * L;
            atomicAdd(&acc[(size_t)l * H + h], w);
        }
    } else if (live) {
        const uint32_t h = c / L, l = c - h * L;
        atomicAdd(&acc[(size_t)l * H + h], w);
    }
}

// Stored alignment values (files saved with incidence_only = False, legacy COO files): EMfactory.prepare
// normalises them per read and sums them per column (EMfactory.py:95-98), once; every later E-step
// starts from ones again (Sparse3DMatrix.reset).  den[r] = sum of the row's values, then
// acc[l][h] += count[r] * value / den[r].
__global__ void __launch_bounds__(256)
csc_den_values_kernel(uint64_t n, const uint32_t *__restrict__ ent_row, const double *__restrict__ vals,
                      double *__restrict__ den) {
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n) atomicAdd(&den[ent_row[k]], vals[k]);
}

__global__ void __launch_bounds__(256)
csc_acc_values_kernel(uint64_t n, uint32_t ncols, uint32_t L, uint32_t H, const uint64_t *__restrict__ col_ptr,
                      const uint32_t *__restrict__ ent_row, const double *__restrict__ vals,
                      const double *__restrict__ count, const double *__restrict__ den, double *__restrict__ acc,
                      int *__restrict__ bad) {
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k - (threadIdx.x & 63) >= n) return;
    const bool live = k < n;
    const uint32_t c = entry_column(col_ptr, ncols, live ? k : n - 1, n);
    if (!live) return;
    const uint32_t r = ent_row[k];
    const double d = den[r];
    if (!(d > 0.0) || !(vals[k] >= 0.0)) { *bad = 1; return; }
    const uint32_t h = c / L, l = c - h * L;
    atomicAdd(&acc[(size_t)l * H + h], (count ? count[r] : 1.0) * vals[k] / d);
}

// `-G` haplotype mask (gbrs/emase_utils.py:240-273: multiply(gtmask, axis=2) + eliminate_zeros): the mask is
// per (haplotype, locus), i.e. it drops whole CSC columns, so the masked tensor is the kept columns moved up
// against each other.  dst_ptr are the column offsets after the mask (dropped columns have width 0), src_ptr the
// offsets in the arrays as uploaded; one thread per surviving entry.
template <typename T>
__global__ void __launch_bounds__(256)
compact_columns_kernel(uint64_t n, uint32_t ncols, const uint64_t *__restrict__ dst_ptr,
                       const uint64_t *__restrict__ src_ptr, const T *__restrict__ src, T *__restrict__ dst) {
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k - (threadIdx.x & 63) >= n) return;
    const bool live = k < n;
    const uint32_t c = entry_column(dst_ptr, ncols, live ? k : n - 1, n);
    if (live) dst[k] = src[src_ptr[c] + (k - dst_ptr[c])];
}

// largest row id of the uploaded arrays (inputs that arrive as device pointers cannot be checked on
// the host, and an out-of-range id would make the scatter kernels fault)
__global__ void __launch_bounds__(256)
max_row_kernel(uint64_t n, const uint32_t *__restrict__ ent_row, unsigned int *__restrict__ out) {
    unsigned int m = 0;
    for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (uint64_t)gridDim.x * blockDim.x)
        m = max(m, ent_row[k]);
    for (int off = 32; off > 0; off >>= 1) m = max(m, (unsigned int)__shfl_down((int)m, off, WAVE));
    if ((threadIdx.x & 63) == 0) atomicMax(out, m);
}

// `--report-alignment-counts` on the CSC arrays (AlignmentPropertyMatrix.py:389-459).
//   nnz_row[r]   number of stored entries of row r   (sum LOCUS then HAPLOTYPE)
//   nloc_row[r]  number of distinct loci of row r    (nnz of the HAPLOTYPE-summed matrix)
__global__ void __launch_bounds__(256)
csc_rowstat_kernel(uint64_t n, uint32_t ncols, uint32_t L, const uint64_t *__restrict__ col_ptr,
                   const uint32_t *__restrict__ ent_row, uint32_t *__restrict__ nnz_row) {
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n) atomicAdd(&nnz_row[ent_row[k]], 1u);
}

// ------------------------------------------------------------------------------------------
// Read-level posteriors (gbrs_em_posterior, GBRS_EM_POSTERIOR).  The E-steps above never form the posterior of a
// stored entry; these passes do, after the fact, on the kept CSC arrays and the theta the last step started from, so
// the result is the same whichever layout the EM itself ran on.
// ------------------------------------------------------------------------------------------

// theta before a step.  Launched behind the previous step's error pass, so a step that the stopping rule turned into
// a no-op leaves the kept theta alone, as it leaves theta alone.
__global__ void __launch_bounds__(256)
keep_theta_kernel(uint64_t n, const double *__restrict__ theta, double *__restrict__ kept,
                  const EmScalars *__restrict__ sc) {
    if (sc->stop) return;
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) kept[i] = theta[i];
}

// Model 4: D_r = sum of the kept theta over the read's entries (csc_den_kernel on the kept theta, no stop flag)
__global__ void __launch_bounds__(256)
post_den_kernel(uint64_t n, uint32_t ncols, uint32_t L, uint32_t H, const uint64_t *__restrict__ col_ptr,
                const uint32_t *__restrict__ ent_row, const double *__restrict__ kept, double *__restrict__ den) {
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k - (threadIdx.x & 63) >= n) return;
    const bool live = k < n;
    const uint32_t c = entry_column(col_ptr, ncols, live ? k : n - 1, n);
    if (!live) return;
    const uint32_t h = c / L, l = c - h * L;
    atomicAdd(&den[ent_row[k]], kept[(size_t)l * H + h]);
}

// One double per entry of haplotype `hap`: the entries [k0, k1) of the CSC arrays, out[k - k0].  A wavefront holds 64
// consecutive entries, nearly always of one column (entry_column), so theta is one broadcast load, the row ids and
// the output are coalesced streams and the denominators (model 4) or the step's factors (models 1-3) the gather.
//   model 4     theta / D_r
//   models 1-3  theta * fac / count[r]: model_row_kernel stored fac = count[r] f / D_r at the entry (0 where theta is 0)
template <bool MODEL4>
__global__ void __launch_bounds__(256)
post_value_kernel(uint64_t k0, uint64_t k1, uint32_t ncols, uint32_t L, uint32_t H, uint32_t hap,
                  const uint64_t *__restrict__ col_ptr, const uint32_t *__restrict__ ent_row,
                  const double *__restrict__ kept, const double *__restrict__ den, const double *__restrict__ fac,
                  const double *__restrict__ count, double *__restrict__ out) {
    const uint64_t k = k0 + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k - (threadIdx.x & 63) >= k1) return;
    const bool live = k < k1;
    const uint32_t c = entry_column(col_ptr, ncols, live ? k : k1 - 1, k1);
    if (!live) return;
    const uint32_t l = c - hap * L;
    const double t = kept[(size_t)l * H + hap];
    const uint32_t r = ent_row[k];
    double v;
    if (MODEL4) v = t == 0.0 ? 0.0 : t / den[r];
    else v = t * (fac[k] / (count ? count[r] : 1.0));
    out[k - k0] = v;
}

#include "em_tiles.inc"
#include "em_models.inc"
#include "em_resample.inc"

}  // namespace gbrs

using namespace gbrs;

// ------------------------------------------------------------------------------------------
// Handle
// ------------------------------------------------------------------------------------------

struct gbrs_em {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = true;
    uint64_t R = 0, N = 0;
    uint32_t L = 0, H = 0;
    bool has_count = false, has_len = false, prepared = false;
    uint32_t flags = 0;

    int layout = 0;               // 0 = csc-direct, 1 = packed row tiles
    EmPlan plan;                  // what create resolved (em_plan.h); a pass's route is resolved from it (em_step.h, em_route)
    bool acc_external = false;    // the caller all-reduces acc (sharded): always materialise all of it
    TileLayout tl;

    // layout 0
    DevBuf<uint32_t> ent_row;
    DevBuf<uint64_t> col_ptr;     // H*L + 1
    DevBuf<uint64_t> col_ptr_src; // H*L + 1: column offsets of the caller's arrays when a haplotype mask dropped columns
    bool masked = false;          // (kept with GBRS_EM_KEEP_CSC, for gbrs_em_set_initial_values)
    DevBuf<double> den;           // R

    DevBuf<double> count, eff_len;                 // R ; L*H locus-major
    DevBuf<double> acc_init;                       // L*H: prepare()'s column sums when the file stores values
    bool has_init = false, keep_csc = false;
    bool stopped = false;          // the device's stop flag is set: every step kernel is a no-op until it is cleared
    DevBuf<double> theta, acc, counts;             // L*H locus-major
    bool counts_stale = false;                     // the fused M-step ran since `counts` was written (em_refresh_counts)
    DevBuf<double> tot_prev, tot_new;              // L
    DevBuf<double> partials;                       // 3 * RED_BLOCKS (pseudocount reductions)
    DevBuf<double> msums;                          // M-step block sums [2][msum_cap] + ERR_BLOCKS error partials
    uint32_t msum_cap = 0, msum_blocks = 0;        // capacity; workgroups of the last M-step launch
    DevBuf<double> scratch_hl;                     // L*H staging for host <-> device transposes
    DevBuf<double> err_hist;
    DevBuf<EmScalars> scalars;
    int err_hist_cap = 0;
    double last_estep_ms = 0.0, last_step_ms = 0.0;   // means over the steps of the last call
    bool time_steps = true;
    // The error pass of a step may be deferred into the gather launch of the next step (it runs there
    // on extra workgroups beside the gather's, one launch and ~9 us less per iteration); it is
    // flushed as its own launch before anything reads the scalars.
    bool err_pending = false;
    double err_pending_target = -1.0;
    std::vector<hipEvent_t> ev_pool;          // 3 events per timed step of a call (em_one_step); create makes the first 3

    // Pair mode (gbrs_em_pair_*): this handle and a partner hold the two locus ranges of one sample; the stopping rule is
    // evaluated over both on the device.  The first handle of the pair owns the state.
    struct PairScalars { int iters, stop; double err; };
    DevBuf<PairScalars> pair_sc;
    DevBuf<double> pair_hist;
    int pair_hist_cap = 0;
    hipEvent_t pair_ev_mstep = nullptr;    // recorded after every M-step of a handle in pair mode
    hipEvent_t pair_ev_err = nullptr;      // recorded after the pair's error pass (first handle)

    // Multiread models 1-3 (gbrs_em_set_groups, em_models.inc).  Genes: the groups, then every locus in no group as a
    // gene of its own; members ascending.  rank_* map a column h*L + l to its place in the sort order of model 1
    // (gene, haplotype, locus) and of models 2/3 (gene, locus, haplotype); inv_* map it back to l*32 + h.
    bool grouped = false;
    uint32_t n_genes = 0;
    DevBuf<uint32_t> gene_ptr, gene_mem, locus_gene, row_ptr;
    DevBuf<uint32_t> rank_m1, inv_m1, rank_m23, inv_m23;
    GroupedOrder order_m1, order_m23;               // built at the first step of a model that uses it
    DevBuf<double> gene_tot, gene_hap_tot, locus_tot, fac;   // T (genes), Y (genes x H), U (L), per-entry factors (N)

    // Read-level posteriors (GBRS_EM_POSTERIOR, gbrs_em_posterior): theta before the last step, the per-read
    // denominators of that step (model 4; made at the first request after it) and one haplotype's values.
    DevBuf<double> theta_kept, post_den, post_vals;  // L*H locus-major ; R ; the longest haplotype's entries
    int post_model = 0;                              // model of the last step through gbrs_em_step / _step_model / _run; 0: none
    bool post_den_valid = false;

    // Bootstrap replicates (GBRS_EM_RESAMPLE, em_resample.inc).  `count` holds the CURRENT row weights (what the CSC,
    // models 1-3 and posterior kernels read); base_count the file's counts as integers (absent: every row counts once);
    // big_rows the rows whose count is above resample_cut (a workgroup each in the draw).
    bool resample = false, has_base = false;
    DevBuf<uint32_t> base_count, big_rows;
    uint32_t n_big = 0;
    // replicate statistics (gbrs_em_bootstrap_begin / _add / _get): level 0 isoforms, 1 genes; quantity 0 TPM, 1 counts
    struct Stats {
        bool active = false;
        uint32_t n = 0;
        int64_t G = 0;
        DevBuf<int64_t> gptr, gmem;
        DevBuf<double> theta_sum;
        DevBuf<double> cur[2][2], mean[2][2], m2[2][2], tot_mean[2][2], tot_m2[2][2];
    } stats;

    // The gather-side M-step (em_step.h em_gather_mstep, em_gather_steps below): three A vectors in rotation (`acc` and
    // these two), a second theta, second totals and block sums.  Made at the first call that takes the route.
    struct Gather {
        bool ready = false;
        DevBuf<double> acc_b[2], theta_b, tot_prev_b, tot_new_b, msums_b;
        int rot = 0;             // the A vector the next launch adds into; its several-slot rows are zero (clean)
        bool clean = false;      // the A invariant holds and the totals of the loci without a slot are 0 in both sets
        bool primed = false;     // theta of the loci without a slot is 0: an M-step has run since theta was last set
        std::vector<const double *> wrote;   // last call: wrote[m], the vector that holds theta of its iteration m (0: at its start)
    } gm;

    int red_blocks() const { return (int)std::min<uint64_t>(RED_BLOCKS, (L + RED_THREADS - 1) / RED_THREADS); }
};

// gbrs_counts_*: the alignments of `--report-alignment-counts` on the device, and the workspace of the last get
struct gbrs_counts {
    int device = 0;
    uint64_t R = 0, n = 0;
    uint32_t L = 0, H = 0;
    gbrs::DevBuf<uint32_t> ent_row;
    gbrs::DevBuf<uint64_t> col_ptr;
    gbrs::DevBuf<double> d_count;
    hipStream_t s = nullptr;
    gbrs::CountsWork *work = nullptr;
};

namespace {

// ---- the error pass -----------------------------------------------------------------------------------------------------
ErrArgs em_err_args(gbrs_em *em, double target_err) {
    ErrArgs ea;
    ea.L = em->L;
    ea.nblocks = (int)em->msum_blocks;
    ea.cap = em->msum_cap;
    ea.tot_prev = em->tot_prev.p;
    ea.tot_new = em->tot_new.p;
    ea.partials = em->msums.p;
    ea.sc = em->scalars.p;
    ea.target_err = target_err;
    ea.err_hist = em->err_hist.p;
    ea.err_hist_cap = em->err_hist_cap;
    ea.n_err_blocks = (uint32_t)std::min<uint64_t>(ERR_BLOCKS, (em->L + RED_THREADS - 1) / RED_THREADS);
    return ea;
}

int em_launch_err(gbrs_em *em, double target_err) {
    const ErrArgs ea = em_err_args(em, target_err);
    hipLaunchKernelGGL(err_finish_kernel, dim3(ea.n_err_blocks), dim3(RED_THREADS), 0, em->stream, ea);
    GBRS_HIP_CHECK(hipGetLastError());
    return GBRS_OK;
}

// Runs a deferred error pass now (before anything that reads or resets the step scalars).
int em_flush_err(gbrs_em *em) {
    if (!em->err_pending) return GBRS_OK;
    em->err_pending = false;
    return em_launch_err(em, em->err_pending_target);
}

int em_check_float(gbrs_em *em, EmScalars &host) {
    GBRS_TRY(em_flush_err(em));
    GBRS_HIP_CHECK(hipMemcpyAsync(&host, em->scalars.p, sizeof(EmScalars), hipMemcpyDeviceToHost, em->stream));
    GBRS_HIP_CHECK(hipStreamSynchronize(em->stream));
    em->stopped = host.stop != 0;
    if (host.float_error && !em->plan.no_float_check)
        return fail(GBRS_ERR_FLOAT, "invalid value encountered in divide (a read's alignments all have zero abundance)");
    return GBRS_OK;
}

// ---- one pass: what it launches (em_step.h), then one function per launch ---------------------------------------------------

// The route of a pass of this kind over the handle as it stands.  Resolved once per API call, outside any loop over steps.
EmStepShape em_step_shape(const gbrs_em *em) {
    const TileLayout &tl = em->tl;
    EmStepShape s;
    s.tiled = em->layout == 1;
    s.H = em->H; s.tH = em->plan.tH; s.view = em->plan.view;
    s.no_tiles = tl.n_tiles == 0; s.no_long = tl.n_long == 0; s.no_entries = em->N == 0;
    s.weighted = tl.weighted; s.deterministic = tl.deterministic; s.all_one_word = tl.all_one_word;
    s.persist_groups = em->plan.persist_groups;
    s.acc_handed_out = em->acc_external;
    s.no_fused_mstep = em->plan.no_fused_mstep;
    return s;
}
EmStepRoute em_route(const gbrs_em *em, EmPass pass) { return em_step_route(em_step_shape(em), pass); }

// Tiles -> partials (a locus with a single slot: straight into acc).
template <int HT, bool ONES>
int em_launch_tiles_h(gbrs_em *em, const EmStepRoute &r) {
    const TileLayout &tl = em->tl;
    const uint32_t tH = em->plan.tH;
    // a deferred error pass of the previous step rides on this launch as extra workgroups
    ErrArgs ea = em_err_args(em, em->err_pending_target);
    if (!r.err_rides || !em->err_pending) ea.n_err_blocks = 0;
    em->err_pending = false;
    const dim3 grid((unsigned)tl.n_tiles + ea.n_err_blocks), block(TILE_THREADS);
    const double *ww = tl.weighted ? tl.word_weight.p : (const double *)nullptr;
    const SetArgs sets{em->plan.tL, tl.n_sets ? tl.set_ptr.p : nullptr, tl.set_members.p, tl.dest_list.p, tl.dict_b.p, tl.dest_b.p,
                       em->resample ? 1u : 0u};
    const uint32_t lead_mask = em->plan.lead_mask;
#define GBRS_LAUNCH_TILES(W, D)                                                                                            \
    hipLaunchKernelGGL((tile_estep_kernel<HT, W, ONES, D>), grid, block, 0, em->stream, tH, tl.tiles.p, tl.words.p,        \
                       tl.dict.p, ww, em->theta.p, tl.partials.p, tl.slot_dest.p, em->acc.p, em->scalars.p,               \
                       (uint32_t)tl.n_tiles, ea, sets, lead_mask, GatherArgs{})
    switch (r.estep) {
        case EmEstep::Persistent:
        case EmEstep::PersistentOneWord: {
            // persistent workgroups (em_tiles.inc): as many as the chip holds at once, each walking several tiles with the
            // next tile's header, dictionary and theta fetched under the current tile's batch loop
            const uint32_t G = std::min<uint32_t>(em->plan.persist_groups, (uint32_t)tl.n_tiles);
            const dim3 pgrid(G + ea.n_err_blocks);
#define GBRS_LAUNCH_PERSISTENT(HH, W, OW)                                                                                  \
            hipLaunchKernelGGL((tile_estep_persistent_kernel<HH, W, OW>), pgrid, block, 0, em->stream, tH, tl.tiles.p,     \
                               tl.words.p, tl.dict.p, ww, em->theta.p, tl.partials.p, tl.slot_dest.p,                      \
                               (int64_t)(em->acc.p - tl.partials.p), em->scalars.p, (uint32_t)tl.n_tiles, G, ea, sets)
            if (r.estep == EmEstep::PersistentOneWord) GBRS_LAUNCH_PERSISTENT(HT == 8 ? 8 : 1, false, HT == 8);
            else if (r.weighted) GBRS_LAUNCH_PERSISTENT(HT, true, false);
            else GBRS_LAUNCH_PERSISTENT(HT, false, false);
#undef GBRS_LAUNCH_PERSISTENT
            break;
        }
        case EmEstep::TilesDeterministic:        // fixed-order sums instead of LDS float atomics (GBRS_EM_DETERMINISTIC)
            if (r.weighted) GBRS_LAUNCH_TILES(true, true); else GBRS_LAUNCH_TILES(false, true);
            break;
#if !defined(GBRS_NO_ONEWORD)
        case EmEstep::TilesOneWord:
            // no row of the layout has more than one word (single-locus reads, or locus sets): no row sums at all
            hipLaunchKernelGGL((tile_estep_kernel<HT == 8 ? 8 : 1, false, ONES, false, HT == 8>), grid, block, 0, em->stream, tH,
                               tl.tiles.p, tl.words.p, tl.dict.p, ww, em->theta.p, tl.partials.p, tl.slot_dest.p, em->acc.p,
                               em->scalars.p, (uint32_t)tl.n_tiles, ea, sets, lead_mask, GatherArgs{});
            break;
#endif
        default:
            if (r.weighted) GBRS_LAUNCH_TILES(true, false); else GBRS_LAUNCH_TILES(false, false);
    }
#undef GBRS_LAUNCH_TILES
    return GBRS_OK;
}
int em_launch_tiles(gbrs_em *em, const EmStepRoute &r) {
#define GBRS_TILES_OF(HT) (r.pass == EmPass::Prepare ? em_launch_tiles_h<HT, true>(em, r) : em_launch_tiles_h<HT, false>(em, r))
    switch (r.width) {
        case 1: return GBRS_TILES_OF(1);
        case 2: return GBRS_TILES_OF(2);
        case 4: return GBRS_TILES_OF(4);
        case 8: return GBRS_TILES_OF(8);
        case 16: return GBRS_TILES_OF(16);
        default: return GBRS_TILES_OF(0);
    }
#undef GBRS_TILES_OF
}

// Long rows -> acc_extra.
int em_launch_long_rows(gbrs_em *em, const EmStepRoute &r) {
    const TileLayout &tl = em->tl;
    const bool ones = r.pass == EmPass::Prepare;
    GBRS_HIP_CHECK(hipMemsetAsync(tl.acc_extra.p, 0, tl.acc_extra.bytes(), em->stream));
#define GBRS_LAUNCH_LONG(KERNEL, GRID, BLOCK)                                                                              \
    hipLaunchKernelGGL(KERNEL, GRID, BLOCK, 0, em->stream, tl.n_long, em->plan.tH, tl.long_ptr.p, tl.long_loc.p,          \
                       tl.long_mask.p, tl.long_weight.p, em->theta.p, tl.acc_extra.p, em->scalars.p, em->resample ? 1u : 0u)
    const dim3 grid((unsigned)((tl.n_long + 3) / 4));
    if (r.long_rows == EmLongRows::Serial) {
        if (ones) GBRS_LAUNCH_LONG(long_rows_estep_serial_kernel<true>, dim3(1), dim3(64));
        else GBRS_LAUNCH_LONG(long_rows_estep_serial_kernel<false>, dim3(1), dim3(64));
    } else {
        if (ones) GBRS_LAUNCH_LONG(long_rows_estep_kernel<true>, grid, dim3(256));
        else GBRS_LAUNCH_LONG(long_rows_estep_kernel<false>, grid, dim3(256));
    }
#undef GBRS_LAUNCH_LONG
    return GBRS_OK;
}

// Partials [+ acc_extra] -> acc: the loci the tiles wrote more than one slot for, or every element.
int em_launch_gather(gbrs_em *em, const EmStepRoute &r) {
    const TileLayout &tl = em->tl;
    // (the gather walks the layout's loci: half-loci of tH haplotypes under the half-locus view - the same elements of acc)
    const uint32_t gH = em->plan.tH, gL = em->plan.tL;
    uint32_t HP = 1;
    while (HP < gH) HP <<= 1;
    const bool all = r.gather == EmGather::All;
    const uint64_t elems = all ? (uint64_t)gL * gH : (uint64_t)tl.n_light * gH;
    const unsigned light = (unsigned)((elems + 255) / 256);
    const unsigned heavy = (unsigned)((tl.n_heavy + 3) / 4);
    if (light + heavy > 0)
        hipLaunchKernelGGL(gather_kernel, dim3(light + heavy), dim3(256), 0, em->stream, gL, gH,
                           HP, light, heavy, (uint32_t)tl.n_heavy, all ? 1 : 0, (uint32_t)tl.n_light, tl.light_loci.p,
                           tl.slot_ptr.p, tl.heavy_loci.p, tl.locus_class.p, tl.partials.p,
                           (tl.n_long && all) ? tl.acc_extra.p : (const double *)nullptr, em->acc.p, em->scalars.p,
                           r.pass == EmPass::Prepare ? 0 : 1);
    return GBRS_OK;
}

// E-step on the CSC arrays: acc = A, zero where there is no entry.
template <bool ONES>
int em_launch_csc(gbrs_em *em, const EmStepRoute &r) {
    const uint64_t n = em->N;
    const uint32_t ncols = em->H * em->L;
    GBRS_HIP_CHECK(hipMemsetAsync(em->acc.p, 0, em->acc.bytes(), em->stream));
    if (r.estep != EmEstep::Csc) return GBRS_OK;
    GBRS_HIP_CHECK(hipMemsetAsync(em->den.p, 0, em->den.bytes(), em->stream));
    const unsigned grid = (unsigned)((n + 255) / 256);
    hipLaunchKernelGGL(csc_den_kernel<ONES>, dim3(grid), dim3(256), 0, em->stream, n, ncols, em->L,
                       em->H, em->col_ptr.p, em->ent_row.p, em->theta.p, em->den.p, em->scalars.p);
    hipLaunchKernelGGL(csc_acc_kernel<ONES>, dim3(grid), dim3(256), 0, em->stream, n, ncols, em->L,
                       em->H, em->col_ptr.p, em->ent_row.p, em->has_count ? em->count.p : nullptr,
                       em->den.p, em->acc.p, em->scalars.p, em->resample ? 1u : 0u);
    return GBRS_OK;
}

// E-step of model 1, 2 or 3 (the order must be built): acc = A.
int em_launch_models(gbrs_em *em, int model) {
    const GroupedOrder &o = model == 1 ? em->order_m1 : em->order_m23;
    const uint32_t nt = std::max(em->L, em->n_genes);
    hipLaunchKernelGGL(model_totals_kernel, dim3((nt + 255) / 256), dim3(256), 0, em->stream, em->L, em->H, em->n_genes,
                       em->gene_ptr.p, em->gene_mem.p, em->theta.p, em->gene_tot.p, em->gene_hap_tot.p, em->locus_tot.p,
                       em->scalars.p);
    GBRS_HIP_CHECK(hipMemsetAsync(em->acc.p, 0, em->acc.bytes(), em->stream));
    if (em->N) {
        const dim3 rgrid((unsigned)((em->R + 255) / 256));
        const double *cnt = em->has_count ? em->count.p : (const double *)nullptr;
#define GBRS_LAUNCH_ROWS(M)                                                                                             \
        hipLaunchKernelGGL(model_row_kernel<M>, rgrid, dim3(256), 0, em->stream, em->R, em->H, em->row_ptr.p, o.lh.p,   \
                           o.src.p, em->locus_gene.p, em->theta.p, em->gene_tot.p, em->gene_hap_tot.p, em->locus_tot.p, \
                           cnt, em->fac.p, em->scalars.p)
        if (model == 1) GBRS_LAUNCH_ROWS(1);
        else if (model == 2) GBRS_LAUNCH_ROWS(2);
        else GBRS_LAUNCH_ROWS(3);
#undef GBRS_LAUNCH_ROWS
        hipLaunchKernelGGL(model_col_kernel, dim3((unsigned)((em->N + 255) / 256)), dim3(256), 0, em->stream, em->N,
                           em->H * em->L, em->L, em->H, em->col_ptr.p, em->fac.p, em->acc.p, em->scalars.p);
    }
    GBRS_HIP_CHECK(hipGetLastError());
    return GBRS_OK;
}

// The E-step half of a pass: fills em->acc with A - all of it, or (r.gather) what the M-step that follows does not add up
// itself.  `after_kernels` (nullable) is recorded behind the E-step kernels themselves, before the gather.
int em_estep(gbrs_em *em, const EmStepRoute &r, int model = 4, hipEvent_t after_kernels = nullptr) {
    if (!r.err_rides) GBRS_TRY(em_flush_err(em));        // prepare / no tile launch to ride on
    if (r.estep == EmEstep::Models) GBRS_TRY(em_launch_models(em, model));
    else if (em->layout != 1) GBRS_TRY(r.pass == EmPass::Prepare ? em_launch_csc<true>(em, r) : em_launch_csc<false>(em, r));
    else if (r.estep != EmEstep::None) GBRS_TRY(em_launch_tiles(em, r));
    if (r.long_rows != EmLongRows::None) GBRS_TRY(em_launch_long_rows(em, r));
    if (after_kernels) GBRS_HIP_CHECK(hipEventRecord(after_kernels, em->stream));
    if (r.gather != EmGather::None) GBRS_TRY(em_launch_gather(em, r));
    GBRS_HIP_CHECK(hipGetLastError());
    return GBRS_OK;
}

// The fused launch: the elementwise workgroups take MSTEP_EPT pairs of haplotypes per thread (one haplotype at H = 1),
// a light locus takes H / 2 threads.  msum_cap (gbrs_em_create) covers this grid: it is never larger than one workgroup per
// RED_THREADS elements plus one per RED_THREADS light elements plus one per heavy locus.
template <int H, bool EXTRA, bool LEN>
void em_launch_mstep_gather_h(gbrs_em *em) {
    const TileLayout &tl = em->tl;
    const uint64_t npair = (uint64_t)em->L * MstepRow<H>::LANES, per = (uint64_t)RED_THREADS * MSTEP_EPT;
    const unsigned elem_blocks = (unsigned)((npair + per - 1) / per);
    const unsigned heavy_blocks = (unsigned)tl.n_heavy;         // one workgroup per many-slot locus
    const unsigned light_blocks = (unsigned)((tl.n_light * MstepRow<H>::LANES + RED_THREADS - 1) / RED_THREADS);
    em->msum_blocks = elem_blocks + heavy_blocks + light_blocks;
    hipLaunchKernelGGL((mstep_gather_kernel<H, EXTRA, LEN>), dim3(em->msum_blocks), dim3(RED_THREADS), 0, em->stream, em->L,
                       heavy_blocks, light_blocks, (uint32_t)tl.n_light, tl.heavy_range.p, tl.light_range.p,
                       tl.locus_class.p, tl.partials.p, em->acc.p, EXTRA ? tl.acc_extra.p : (const double *)nullptr,
                       em->theta.p, LEN ? em->eff_len.p : (const double *)nullptr, em->tot_prev.p, em->tot_new.p,
                       em->msums.p, em->msum_cap, em->scalars.p);
}
template <int H>
void em_launch_mstep_gather_opts(gbrs_em *em, bool extra) {
    if (extra) em->has_len ? em_launch_mstep_gather_h<H, true, true>(em) : em_launch_mstep_gather_h<H, true, false>(em);
    else em->has_len ? em_launch_mstep_gather_h<H, false, true>(em) : em_launch_mstep_gather_h<H, false, false>(em);
}
int em_launch_mstep_gather(gbrs_em *em, const EmStepRoute &r) {
    const bool extra = r.long_rows != EmLongRows::None;
    switch (em->H) {
    case 1: em_launch_mstep_gather_opts<1>(em, extra); break;
    case 2: em_launch_mstep_gather_opts<2>(em, extra); break;
    case 4: em_launch_mstep_gather_opts<4>(em, extra); break;
    case 8: em_launch_mstep_gather_opts<8>(em, extra); break;
    case 16: em_launch_mstep_gather_opts<16>(em, extra); break;
    default: return fail(GBRS_ERR_UNSUPPORTED, "the fused M-step has no instance for this haplotype count");
    }
    return GBRS_OK;
}

template <int MODE, int H>
void em_launch_mstep_elem(gbrs_em *em, double *theta, const double *acc, const double *extra, const double *len) {
    const uint64_t npair = (uint64_t)em->L * MstepRow<H>::LANES;
    const unsigned nb = (unsigned)((npair + RED_THREADS - 1) / RED_THREADS);
    em->msum_blocks = nb;
    hipLaunchKernelGGL((mstep_elem_kernel<MODE, H>), dim3(nb), dim3(RED_THREADS), 0, em->stream, em->L, theta, acc,
                       extra, len, em->counts.p, em->tot_prev.p, em->tot_new.p, em->msums.p, em->msum_cap, em->scalars.p);
}
// M-step launch: with the gather, element-parallel (H a power of two) or thread-per-locus.  MODE 1: prepare.
template <int MODE>
int em_launch_mstep_plain(gbrs_em *em, const EmStepRoute &r) {
    const double *len = em->has_len ? em->eff_len.p : nullptr;
    if (r.mstep == EmMstep::PerLocus) {
        const int nb = em->red_blocks();
        em->msum_blocks = nb;
        hipLaunchKernelGGL(mstep_kernel<MODE>, dim3(nb), dim3(RED_THREADS), 0, em->stream, em->L, em->H,
                           em->theta.p, em->acc.p, len, em->counts.p, em->tot_prev.p, em->tot_new.p,
                           em->msums.p, em->msum_cap, em->scalars.p);
        return GBRS_OK;
    }
    const double *extra = r.mstep_adds_extra ? em->tl.acc_extra.p : (const double *)nullptr;
    switch (em->H) {
    case 1: em_launch_mstep_elem<MODE, 1>(em, em->theta.p, em->acc.p, extra, len); break;
    case 2: em_launch_mstep_elem<MODE, 2>(em, em->theta.p, em->acc.p, extra, len); break;
    case 4: em_launch_mstep_elem<MODE, 4>(em, em->theta.p, em->acc.p, extra, len); break;
    case 8: em_launch_mstep_elem<MODE, 8>(em, em->theta.p, em->acc.p, extra, len); break;
    case 16: em_launch_mstep_elem<MODE, 16>(em, em->theta.p, em->acc.p, extra, len); break;
    case 32: em_launch_mstep_elem<MODE, 32>(em, em->theta.p, em->acc.p, extra, len); break;
    default: return fail(GBRS_ERR_UNSUPPORTED, "the element-parallel M-step has no instance for this haplotype count");
    }
    return GBRS_OK;
}
int em_launch_mstep(gbrs_em *em, const EmStepRoute &r) {
    if (r.mstep == EmMstep::Fused) return em_launch_mstep_gather(em, r);
    return r.pass == EmPass::Prepare ? em_launch_mstep_plain<1>(em, r) : em_launch_mstep_plain<0>(em, r);
}

// The expected read counts theta * A of the last iteration (EMfactory.py:302: the last E-step's posterior summed over the
// reads) equal theta' * len, theta' being what that iteration's M-step left: the fused gather + M-step launch does not
// store them (7.7 of its ~55 MB per iteration at C2), they are made from theta when somebody asks (one more rounding:
// within 2 ulp of the product the unfused kernels store).
__global__ void __launch_bounds__(256)
counts_from_theta_kernel(uint64_t n, const double *__restrict__ theta, const double *__restrict__ eff_len, double *__restrict__ counts) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) counts[i] = eff_len ? theta[i] * eff_len[i] : theta[i];
}
int em_refresh_counts(gbrs_em *em) {
    if (!em->counts_stale) return GBRS_OK;
    const uint64_t n = (uint64_t)em->L * em->H;
    hipLaunchKernelGGL(counts_from_theta_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, em->stream, n, em->theta.p,
                       em->has_len ? em->eff_len.p : (const double *)nullptr, em->counts.p);
    GBRS_HIP_CHECK(hipGetLastError());
    em->counts_stale = false;
    return GBRS_OK;
}

// The M-step half of a pass and its error pass.  `defer_err`: leave the error pass to the next pass's tile launch
// (em_launch_tiles_h) or to em_flush_err, where the route allows it.
int em_finish_step(gbrs_em *em, const EmStepRoute &r, double target_err, bool defer_err) {
    GBRS_TRY(em_flush_err(em));
    GBRS_TRY(em_launch_mstep(em, r));
    em->counts_stale = r.counts_stale;
    em->gm.primed = true;        // theta * A: 0 wherever the tiles have no slot
    em->gm.clean = false;        // (acc and the totals are this route's again)
    if (defer_err && r.err_defer) {
        em->err_pending = true;
        em->err_pending_target = target_err;
        return GBRS_OK;
    }
    return em_launch_err(em, target_err);
}

// GBRS_EM_POSTERIOR: theta before the step that is about to be enqueued.  The deferred error pass of the previous step
// runs first, so that the copy sees that step's stop flag.
int em_keep_theta(gbrs_em *em, int model) {
    if (!(em->flags & GBRS_EM_POSTERIOR)) return GBRS_OK;
    GBRS_TRY(em_flush_err(em));
    const uint64_t n = (uint64_t)em->L * em->H;
    hipLaunchKernelGGL(keep_theta_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, em->stream, n, em->theta.p,
                       em->theta_kept.p, em->scalars.p);
    GBRS_HIP_CHECK(hipGetLastError());
    em->post_model = model;
    em->post_den_valid = false;
    return GBRS_OK;
}

// One iteration of `model` (r: EmPass::Step for 4, else EmPass::Model with the order built); `ev` (3 events, nullable)
// times it: ev[1] closes the E-step kernels themselves.  An event record is a barrier packet that costs the queue ~4 us of
// idle time on this hardware, so callers time a sample of the iterations (every EM_TIME_STRIDE-th), not each one.
constexpr int EM_TIME_STRIDE = 8, EM_TIME_SAMPLES = 16;
int em_one_step(gbrs_em *em, const EmStepRoute &r, int model, double target_err, hipEvent_t *ev, bool defer_err) {
    GBRS_TRY(em_keep_theta(em, model));
    if (!em->time_steps) ev = nullptr;
    if (ev) GBRS_HIP_CHECK(hipEventRecord(ev[0], em->stream));
    GBRS_TRY(em_estep(em, r, model, ev ? ev[1] : nullptr));
    GBRS_TRY(em_finish_step(em, r, target_err, defer_err));
    // the tile layout's Model-4 steps write A only for the loci they have sums for and expect 0 elsewhere
    if (r.pass == EmPass::Model && em->layout == 1) GBRS_HIP_CHECK(hipMemsetAsync(em->acc.p, 0, em->acc.bytes(), em->stream));
    if (ev) GBRS_HIP_CHECK(hipEventRecord(ev[2], em->stream));
    return GBRS_OK;
}

// last_estep_ms / last_step_ms: the means over the n timed steps of a call, whose events lead em->ev_pool
void em_read_times(gbrs_em *em, int n) {
    if (!em->time_steps || n <= 0) return;
    double se = 0.0, ss = 0.0;
    for (int i = 0; i < n; ++i) {
        float a = 0.f, b = 0.f;
        if (hipEventElapsedTime(&a, em->ev_pool[3 * i], em->ev_pool[3 * i + 1]) != hipSuccess) return;   // (never recorded)
        if (hipEventElapsedTime(&b, em->ev_pool[3 * i], em->ev_pool[3 * i + 2]) != hipSuccess) return;
        se += a;
        ss += b;
    }
    em->last_estep_ms = se / n;
    em->last_step_ms = ss / n;
}

// ---- the gather-side M-step: iteration n's M-step in launch n + 1's prologues (em_step.h, em_layout.h GatherArgs) -------

// Do this handle's Model-4 steps take the route, as it stands?
bool em_gather_route(const gbrs_em *em) {
    if (em->layout != 1 || em->N == 0) return false;
    const TileLayout &tl = em->tl;
    const EmStepShape s = em_step_shape(em);
    EmGatherShape g;
    g.no_heavy = tl.n_heavy == 0;
    g.n_tiles = (uint32_t)tl.n_tiles; g.tile_waves = TILE_WAVES; g.msum_cap = em->msum_cap;
    g.posterior = (em->flags & GBRS_EM_POSTERIOR) != 0;
    g.resample = em->resample;
    g.pair_mode = em->pair_ev_mstep != nullptr;
    EmTuning t;
    t.no_gather_mstep = em->plan.no_gather_mstep;
    return em_gather_mstep(s, g, EmPass::Step, t);
}

int em_gather_setup(gbrs_em *em) {
    gbrs_em::Gather &gm = em->gm;
    const size_t LH = (size_t)em->L * em->H;
    if (!gm.ready) {
        GBRS_TRY(build_gather_slots(em->tl, em->plan.tL, em->stream));
        for (DevBuf<double> *b : {&gm.acc_b[0], &gm.acc_b[1], &gm.theta_b}) {
            GBRS_TRY(b->alloc(LH));
            GBRS_HIP_CHECK(hipMemsetAsync(b->p, 0, b->bytes(), em->stream));      // (theta_b: the loci without a slot stay 0)
        }
        GBRS_TRY(gm.tot_prev_b.alloc(em->L));
        GBRS_TRY(gm.tot_new_b.alloc(em->L));
        GBRS_TRY(gm.msums_b.alloc(em->msums.n));
        GBRS_HIP_CHECK(hipMemsetAsync(gm.msums_b.p, 0, gm.msums_b.bytes(), em->stream));
        gm.ready = true;
        gm.clean = false;
    }
    if (!gm.clean) {
        // another route has used acc and the totals since (or a stop left a launch half done): the several-slot rows of all
        // three A vectors are zero again, the rotation starts over, and the totals of the loci without a slot are 0
        for (double *p : {em->acc.p, gm.acc_b[0].p, gm.acc_b[1].p}) GBRS_HIP_CHECK(hipMemsetAsync(p, 0, LH * sizeof(double), em->stream));
        for (double *p : {em->tot_prev.p, em->tot_new.p, gm.tot_prev_b.p, gm.tot_new_b.p})
            GBRS_HIP_CHECK(hipMemsetAsync(p, 0, (size_t)em->L * sizeof(double), em->stream));
        gm.rot = 0;
        gm.clean = true;
    }
    return GBRS_OK;
}

template <int HT>
void em_launch_gather_tiles(gbrs_em *em, bool one_word, const double *theta, const ErrArgs &ea, const GatherArgs &ga) {
    const TileLayout &tl = em->tl;
    const dim3 grid((unsigned)tl.n_tiles + ea.n_err_blocks), block(TILE_THREADS);
    const SetArgs sets{em->plan.tL, tl.n_sets ? tl.set_ptr.p : nullptr, tl.set_members.p, tl.dest_list.p, tl.dict_b.p, tl.dest_b.p, 0u};
#define GBRS_LAUNCH_GATHER(OW)                                                                                             \
    hipLaunchKernelGGL((tile_estep_kernel<HT, false, false, false, OW, true>), grid, block, 0, em->stream, em->plan.tH,    \
                       tl.tiles.p, tl.words.p, tl.dict.p, (const double *)nullptr, theta, (double *)nullptr, tl.slot_dest.p, \
                       (double *)nullptr, em->scalars.p, (uint32_t)tl.n_tiles, ea, sets, em->plan.lead_mask, ga)
    if constexpr (HT == 8) {
        if (one_word) { GBRS_LAUNCH_GATHER(true); return; }
    }
    GBRS_LAUNCH_GATHER(false);
#undef GBRS_LAUNCH_GATHER
}

// k iterations (k >= 1) on the route: k launches - the first with theta current, every later one applying the M-step of
// the one before - then the error pass of iteration k - 1, one elementwise M-step on the last A vector and its error pass.
// It leaves the handle as k two-launch steps do: theta current (in em->theta), counts fresh.  ev / stride / timed: as in
// gbrs_em_step (launch 1 + i * stride is timed).  A stop inside the call: em_gather_settle.
int em_gather_steps(gbrs_em *em, int k, double target_err, int stride, int timed) {
    GBRS_TRY(em_flush_err(em));
    GBRS_TRY(em_gather_setup(em));
    gbrs_em::Gather &gm = em->gm;
    const TileLayout &tl = em->tl;
    const EmStepRoute route = em_route(em, EmPass::Step);
    const bool one_word = route.estep == EmEstep::TilesOneWord;
    double *accs[3] = {em->acc.p, gm.acc_b[0].p, gm.acc_b[1].p};
    double *thetas[2] = {em->theta.p, gm.theta_b.p};
    double *tps[2] = {em->tot_prev.p, gm.tot_prev_b.p}, *tns[2] = {em->tot_new.p, gm.tot_new_b.p}, *mss[2] = {em->msums.p, gm.msums_b.p};
    gm.wrote.assign((size_t)k + 1, nullptr);
    gm.wrote[0] = em->theta.p;
    ErrArgs waiting = em_err_args(em, target_err);     // the error pass of the last M-step a launch applied
    waiting.nblocks = (int)(tl.n_tiles * TILE_WAVES);
    const uint32_t n_err = waiting.n_err_blocks;
    bool have_waiting = false;
    int src = 0;
    if (!em->time_steps) timed = 0;
    for (int j = 1; j <= k; ++j) {
        const bool pending = j > 1;
        const int set = j & 1, dst = src ^ 1;
        GatherArgs ga;
        ga.acc_old = accs[(gm.rot + 2) % 3];
        ga.eff_len = em->has_len ? em->eff_len.p : nullptr;
        ga.theta_new = thetas[dst];
        ga.tot_prev = tps[set]; ga.tot_new = tns[set]; ga.msums = mss[set]; ga.cap = em->msum_cap;
        ga.acc_cur = accs[gm.rot]; ga.acc_next = accs[(gm.rot + 1) % 3];
        ga.gdest = tl.gdest.p; ga.gdest_b = tl.gdest_b.p; ga.gdest_list = tl.gdest_list.p;
        ga.pending = pending ? 1u : 0u;
        ErrArgs ea = waiting;
        ea.n_err_blocks = have_waiting ? n_err : 0u;
        const int slot = (j - 1) / stride;
        hipEvent_t *ev = ((j - 1) % stride == 0 && slot < timed) ? &em->ev_pool[3 * slot] : nullptr;
        if (ev) GBRS_HIP_CHECK(hipEventRecord(ev[0], em->stream));
        switch (em->H) {
        case 1: em_launch_gather_tiles<1>(em, one_word, thetas[src], ea, ga); break;
        case 2: em_launch_gather_tiles<2>(em, one_word, thetas[src], ea, ga); break;
        case 4: em_launch_gather_tiles<4>(em, one_word, thetas[src], ea, ga); break;
        case 8: em_launch_gather_tiles<8>(em, one_word, thetas[src], ea, ga); break;
        default: return fail(GBRS_ERR_UNSUPPORTED, "the gather-side M-step has no instance for this haplotype count");
        }
        if (ev) {
            GBRS_HIP_CHECK(hipEventRecord(ev[1], em->stream));
            GBRS_HIP_CHECK(hipEventRecord(ev[2], em->stream));
        }
        if (pending) {
            gm.wrote[j - 1] = thetas[dst];
            waiting.tot_prev = tps[set]; waiting.tot_new = tns[set]; waiting.partials = mss[set];
            have_waiting = true;
            src = dst;
        }
        gm.rot = (gm.rot + 1) % 3;
    }
    GBRS_HIP_CHECK(hipGetLastError());
    if (have_waiting) {
        waiting.n_err_blocks = n_err;
        hipLaunchKernelGGL(err_finish_kernel, dim3(n_err), dim3(RED_THREADS), 0, em->stream, waiting);
    }
    // M(k), in place on the vector that holds theta of iteration k - 1, from the A vector the last launch added into
    {
        double *theta = thetas[src];
        const double *acc = accs[(gm.rot + 2) % 3], *len = em->has_len ? em->eff_len.p : nullptr;
        switch (em->H) {
        case 1: em_launch_mstep_elem<0, 1>(em, theta, acc, nullptr, len); break;
        case 2: em_launch_mstep_elem<0, 2>(em, theta, acc, nullptr, len); break;
        case 4: em_launch_mstep_elem<0, 4>(em, theta, acc, nullptr, len); break;
        default: em_launch_mstep_elem<0, 8>(em, theta, acc, nullptr, len); break;      // (1, 2, 4, 8: checked at the launches above)
        }
    }
    gm.wrote[k] = thetas[src];
    if (src == 1) em->theta.swap(gm.theta_b);
    em->counts_stale = false;
    GBRS_TRY(em_launch_err(em, target_err));
    GBRS_HIP_CHECK(hipGetLastError());
    return GBRS_OK;
}

// After a batch of k gather-side iterations that began at iters_done = it0 and met the stopping rule at iteration `done`
// (device scalars read, stream idle): the error pass of iteration m = done - it0 raised the flag while launch m + 2 was
// running or before it, so theta of iteration m - stored by launch m + 1, or by the closing M-step when m = k - is intact
// in its vector while the other one may hold a part of iteration m + 1.  That vector becomes em->theta (a swap, no copy).
void em_gather_settle(gbrs_em *em, int it0, int done) {
    gbrs_em::Gather &gm = em->gm;
    const int k = (int)gm.wrote.size() - 1, m = done - it0;
    // m = k: the call ran to its end and left theta current itself.  m = 0: the flag was up before the call began, every
    // launch of it was a no-op, and theta is still in the vector the call started from (wrote[0]) - settled like any m < k,
    // because the call's closing swap may have made the other vector current.
    if (k < 1 || m < 0 || m >= k) return;
    if (gm.wrote[m] != em->theta.p) em->theta.swap(gm.theta_b);
    em->counts_stale = true;                       // the closing M-step stored nothing: counts are theta * len when asked for
    gm.clean = false;                              // launch m + 2 may have added into and zeroed a part of its A vectors
}

int em_finish_prepare(gbrs_em *em, double pseudocount) {
    GBRS_TRY(em_launch_mstep(em, em_route(em, EmPass::Prepare)));
    em->counts_stale = false;
    const int nb = em->red_blocks();
    if (pseudocount > 0.0) {
        hipLaunchKernelGGL(pseudo_add_kernel, dim3(nb), dim3(RED_THREADS), 0, em->stream, em->L,
                           em->H, pseudocount, em->theta.p, em->partials.p);
        hipLaunchKernelGGL(pseudo_scale_kernel, dim3(nb), dim3(RED_THREADS), 0, em->stream,
                           (uint64_t)em->L * em->H, nb, em->theta.p, em->partials.p, em->scalars.p);
    }
    GBRS_HIP_CHECK(hipMemsetAsync(em->partials.p, 0, em->partials.bytes(), em->stream));
    // A of the loci without any slot must read 0 in the steps (the tile path then writes only the loci
    // it has rows for); prepare's full gather left the long rows' contribution there
    GBRS_HIP_CHECK(hipMemsetAsync(em->acc.p, 0, em->acc.bytes(), em->stream));
    GBRS_HIP_CHECK(hipGetLastError());
    em->prepared = true;
    em->gm.primed = em->gm.clean = false;     // (the loci without reads carry theta again)
    return GBRS_OK;
}

int em_reset_scalars(gbrs_em *em, bool keep_iters) {
    GBRS_TRY(em_flush_err(em));
    EmScalars host;
    std::memset(&host, 0, sizeof(host));
    if (keep_iters) {
        EmScalars cur;
        GBRS_HIP_CHECK(hipMemcpyAsync(&cur, em->scalars.p, sizeof(cur), hipMemcpyDeviceToHost, em->stream));
        GBRS_HIP_CHECK(hipStreamSynchronize(em->stream));
        host.iters_done = cur.iters_done;
    }
    em->stopped = false;
    GBRS_HIP_CHECK(hipMemcpyAsync(em->scalars.p, &host, sizeof(host), hipMemcpyHostToDevice, em->stream));
    GBRS_HIP_CHECK(hipStreamSynchronize(em->stream));
    return GBRS_OK;
}

int em_ensure_hist(gbrs_em *em, int cap) {
    if (cap <= em->err_hist_cap) return GBRS_OK;
    GBRS_HIP_CHECK(hipStreamSynchronize(em->stream));
    GBRS_TRY(em->err_hist.alloc((size_t)cap));
    em->err_hist_cap = cap;
    return GBRS_OK;
}

// ---- multiread models 1-3 (em_models.inc) ------------------------------------------------------------------------
int em_check_model(const gbrs_em *em, int model) {
    if (model < 1 || model > 4) return fail(GBRS_ERR_INVALID, "The read normalization model should be 1, 2, 3, or 4.");
    if (model == 4) return GBRS_OK;
    if (em->flags & GBRS_EM_DETERMINISTIC)
        return fail(GBRS_ERR_UNSUPPORTED, "multiread model %d has no bit-reproducible form (GBRS_EM_DETERMINISTIC)", model);
    if (!em->grouped)
        return fail(GBRS_ERR_UNSUPPORTED, "multiread model %d needs gene groups: create the handle with "
                                          "GBRS_EM_GROUPED_MODELS and call gbrs_em_set_groups", model);
    return GBRS_OK;
}

int em_ensure_order(gbrs_em *em, int model) {
    GroupedOrder &o = model == 1 ? em->order_m1 : em->order_m23;
    if (o.built) return GBRS_OK;
    GBRS_TRY(em_flush_err(em));
    return build_grouped_order(o, em->R, em->L, em->H, em->N, em->ent_row.p, em->col_ptr.p,
                               model == 1 ? em->rank_m1.p : em->rank_m23.p, model == 1 ? em->inv_m1.p : em->inv_m23.p,
                               em->stream);
}

// Concatenate the per-haplotype CSC arrays on the device: column id c = h*L + l, col_ptr[c] is the
// offset of the column's first entry in ent_row.  Validates monotone indptr and (host inputs) row ids.
// allowed (host, nullable): uint32[L], bit h set = the entries of (haplotype h, locus l) stay; the other columns
// are dropped on the device (compact_columns_kernel).  src_ptr_dev (nullable) then receives the column offsets of
// the arrays as given, for callers that have to move a second per-entry array the same way.
int upload_csc(uint64_t R, uint32_t L, uint32_t H, const uint32_t *const *indptr,
               const uint32_t *const *indices, bool on_device, DevBuf<uint32_t> &ent_row,
               DevBuf<uint64_t> &col_ptr_dev, uint64_t &n_out, const uint32_t *allowed = nullptr,
               DevBuf<uint64_t> *src_ptr_dev = nullptr, hipStream_t stream = nullptr) {
    const hipMemcpyKind kind = on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    std::vector<uint64_t> col_ptr((size_t)H * L + 1), src_ptr;
    if (allowed) src_ptr.resize((size_t)H * L + 1);
    std::vector<uint32_t> tmp(L + 1);
    uint64_t n = 0, n_src = 0;
    std::vector<uint64_t> hap_off(H + 1);
    for (uint32_t h = 0; h < H; ++h) {
        if (!indptr[h]) return fail(GBRS_ERR_INVALID, "indptr[%u] is NULL", h);
        if (on_device) {
            GBRS_HIP_CHECK(hipMemcpy(tmp.data(), indptr[h], (L + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost));
        } else {
            std::memcpy(tmp.data(), indptr[h], (L + 1) * sizeof(uint32_t));
        }
        if (tmp[0] != 0) return fail(GBRS_ERR_INVALID, "indptr[%u][0] != 0", h);
        hap_off[h] = n_src;
        for (uint32_t l = 0; l < L; ++l) {
            if (tmp[l + 1] < tmp[l]) return fail(GBRS_ERR_INVALID, "indptr[%u] is not non-decreasing at %u", h, l);
            col_ptr[(size_t)h * L + l] = n;
            if (allowed) {
                src_ptr[(size_t)h * L + l] = n_src + tmp[l];
                if ((allowed[l] >> h) & 1u) n += tmp[l + 1] - tmp[l];
            } else {
                n += tmp[l + 1] - tmp[l];
            }
        }
        n_src += tmp[L];
    }
    hap_off[H] = n_src;
    col_ptr[(size_t)H * L] = n;
    GBRS_TRY(col_ptr_dev.alloc(col_ptr.size()));
    GBRS_HIP_CHECK(hipMemcpy(col_ptr_dev.p, col_ptr.data(), col_ptr_dev.bytes(), hipMemcpyHostToDevice));
    GBRS_TRY(ent_row.alloc(std::max<uint64_t>(n, 1)));
    DevBuf<uint32_t> staged;                      // masked: the arrays as given, before the columns move up
    DevBuf<uint64_t> src_local;
    if (allowed) {
        src_ptr[(size_t)H * L] = n_src;
        GBRS_TRY(staged.alloc(std::max<uint64_t>(n_src, 1)));
        DevBuf<uint64_t> &sp = src_ptr_dev ? *src_ptr_dev : src_local;
        GBRS_TRY(sp.alloc(src_ptr.size()));
        GBRS_HIP_CHECK(hipMemcpy(sp.p, src_ptr.data(), sp.bytes(), hipMemcpyHostToDevice));
    }
    uint32_t *dst = allowed ? staged.p : ent_row.p;
    for (uint32_t h = 0; h < H; ++h) {
        const uint64_t cnt = hap_off[h + 1] - hap_off[h];
        if (cnt == 0) continue;
        if (!indices[h]) return fail(GBRS_ERR_INVALID, "indices[%u] is NULL", h);
        GBRS_HIP_CHECK(hipMemcpy(dst + hap_off[h], indices[h], cnt * sizeof(uint32_t), kind));
    }
    if (allowed && n) {
        const DevBuf<uint64_t> &sp = src_ptr_dev ? *src_ptr_dev : src_local;
        hipLaunchKernelGGL(compact_columns_kernel<uint32_t>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, n,
                           H * L, col_ptr_dev.p, sp.p, staged.p, ent_row.p);
        GBRS_HIP_CHECK(hipStreamSynchronize(stream));
        GBRS_HIP_CHECK(hipGetLastError());
    }
    n_out = n;
    return GBRS_OK;
}

// Row ids of uploaded CSC arrays are range-checked on the device before any kernel indexes per-row
// storage with them (host and device inputs alike).
int check_row_ids(uint64_t n, const uint32_t *ent_row, uint64_t R, hipStream_t stream) {
    if (n == 0) return GBRS_OK;
    DevBuf<unsigned int> d_max;
    GBRS_TRY(d_max.alloc(1));
    GBRS_HIP_CHECK(hipMemsetAsync(d_max.p, 0, sizeof(unsigned int), stream));
    hipLaunchKernelGGL(max_row_kernel, dim3(1024), dim3(256), 0, stream, n, ent_row, d_max.p);
    unsigned int mx = 0;
    GBRS_HIP_CHECK(hipMemcpyAsync(&mx, d_max.p, sizeof(mx), hipMemcpyDeviceToHost, stream));
    GBRS_HIP_CHECK(hipStreamSynchronize(stream));
    if (mx >= R) return fail(GBRS_ERR_INVALID, "indices hold row id %u >= num_rows", mx);
    return GBRS_OK;
}

int em_create_impl(uint64_t R, uint32_t L, uint32_t H, const uint32_t *const *indptr,
                   const uint32_t *const *indices, const double *count, const double *eff_len,
                   const uint32_t *allowed, int device, uint32_t flags, bool on_device, gbrs_em_t **out) {
    RoctxRange roctx_range("gbrs_em_create");
    if (!out) return fail(GBRS_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (H < 1 || H > 32 || L < 1 || R < 1 || R > 0xFFFFFFFFull)
        return fail(GBRS_ERR_INVALID, "The shape must be a tuple of three positive integers (H <= 32, R < 2^32).");
    if (!indptr || !indices) return fail(GBRS_ERR_INVALID, "indptr/indices tables are NULL");
    const bool resample = (flags & GBRS_EM_RESAMPLE) != 0;
    if (resample && (flags & (GBRS_EM_MERGE_IDENTICAL_ROWS | GBRS_EM_SIDE_BY_SIDE)))
        return fail(GBRS_ERR_UNSUPPORTED, "GBRS_EM_RESAMPLE draws a weight per file row: not available with "
                                          "GBRS_EM_MERGE_IDENTICAL_ROWS or GBRS_EM_SIDE_BY_SIDE");
    GBRS_TRY(select_device(device));
    gbrs_em *em = new gbrs_em();
    struct Guard { gbrs_em *p; ~Guard() { if (p) gbrs_em_destroy(p); } } guard{em};
    em->device = device;
    em->R = R; em->L = L; em->H = H; em->flags = flags;
    em->has_count = count != nullptr || resample;       // (a resampling handle is a weighted one: base weights of count or ones)
    em->resample = resample;
    em->has_base = resample && count != nullptr;
    em->has_len = eff_len != nullptr;
    GBRS_HIP_CHECK(hipStreamCreateWithFlags(&em->stream, hipStreamDefault));
    for (int i = 0; i < 3; ++i) {
        em->ev_pool.push_back(nullptr);
        GBRS_HIP_CHECK(hipEventCreate(&em->ev_pool.back()));
    }
    const hipMemcpyKind kind = on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    uint64_t n = 0;
    StageTimer stg("create");
    em->masked = allowed != nullptr;
    GBRS_TRY(upload_csc(R, L, H, indptr, indices, on_device, em->ent_row, em->col_ptr, n, allowed,
                        (allowed && (flags & GBRS_EM_KEEP_CSC)) ? &em->col_ptr_src : nullptr, em->stream));
    stg.mark("upload csc");
    em->N = n;
    // everything that is known before the build: em_plan.h (the tuning variables are read here, once per create)
    EmShape shape;
    shape.H = H; shape.L = L; shape.R = R; shape.N = n; shape.flags = flags; shape.counts_given = count != nullptr;
    GBRS_HIP_CHECK(hipDeviceGetAttribute(&shape.n_cu, hipDeviceAttributeMultiprocessorCount, device));
    shape.tile_words = TILE_WORDS; shape.tile_words_max = TILE_WORDS_MAX; shape.tile_rounds_min = TILE_ROUNDS_MIN;
    shape.err_blocks = (uint32_t)std::min<uint64_t>(ERR_BLOCKS, ((uint64_t)L + RED_THREADS - 1) / RED_THREADS);   // (estep_err_args)
    if (H <= 16) shape.dict = dict_limits(em_weighted(flags, count != nullptr), (int)H);     // (more: the CSC kernels)
    if (H == 16) shape.dict_half = dict_limits(false, 8);
    const EmPlan &plan = em->plan = em_plan(shape, em_tuning_from_env());
    const size_t LH = (size_t)L * H;
    GBRS_TRY(em->den.alloc(R));
    GBRS_TRY(em->theta.alloc(LH));
    GBRS_TRY(em->acc.alloc(LH));
    GBRS_TRY(em->counts.alloc(LH));
    GBRS_TRY(em->scratch_hl.alloc(LH));
    GBRS_TRY(em->tot_prev.alloc(L));
    GBRS_TRY(em->tot_new.alloc(L));
    GBRS_TRY(em->partials.alloc(3 * RED_BLOCKS));
    em->msum_cap = (uint32_t)(((uint64_t)L * H + RED_THREADS - 1) / RED_THREADS * 2 + L + RED_BLOCKS);   // elementwise + light workgroups + one per many-slot locus
    GBRS_TRY(em->msums.alloc(2 * (size_t)em->msum_cap + ERR_BLOCKS));
    GBRS_TRY(em->scalars.alloc(1));
    if (flags & GBRS_EM_POSTERIOR) {
        GBRS_TRY(em->theta_kept.alloc(LH));
        GBRS_TRY(em->post_den.alloc(R));
    }
    GBRS_HIP_CHECK(hipMemset(em->scalars.p, 0, sizeof(EmScalars)));
    GBRS_HIP_CHECK(hipMemset(em->theta.p, 0, em->theta.bytes()));
    GBRS_HIP_CHECK(hipMemset(em->acc.p, 0, em->acc.bytes()));
    GBRS_HIP_CHECK(hipMemset(em->partials.p, 0, em->partials.bytes()));
    GBRS_HIP_CHECK(hipMemset(em->msums.p, 0, em->msums.bytes()));
    GBRS_HIP_CHECK(hipMemset(em->counts.p, 0, em->counts.bytes()));
    if (count || resample) GBRS_TRY(em->count.alloc(R));
    if (count) GBRS_HIP_CHECK(hipMemcpy(em->count.p, count, R * sizeof(double), kind));
    if (resample) {
        const unsigned rgrid = (unsigned)((R + 255) / 256);
        if (count) {
            DevBuf<int> bad;
            GBRS_TRY(bad.alloc(1));
            GBRS_TRY(em->base_count.alloc(R));
            GBRS_HIP_CHECK(hipMemsetAsync(bad.p, 0, sizeof(int), em->stream));
            hipLaunchKernelGGL(resample_base_kernel, dim3(rgrid), dim3(256), 0, em->stream, R, em->count.p, em->base_count.p, bad.p);
            int hbad = 0;
            GBRS_HIP_CHECK(hipMemcpyAsync(&hbad, bad.p, sizeof(int), hipMemcpyDeviceToHost, em->stream));
            GBRS_HIP_CHECK(hipStreamSynchronize(em->stream));
            if (hbad)
                return fail(GBRS_ERR_INVALID, "GBRS_EM_RESAMPLE needs integer counts in [0, 2^32): a row is drawn count[r] times");
            DevBuf<uint32_t> n_big;
            GBRS_TRY(n_big.alloc(1));
            for (int pass = 0; pass < 2; ++pass) {
                GBRS_HIP_CHECK(hipMemsetAsync(n_big.p, 0, 4, em->stream));
                hipLaunchKernelGGL(resample_big_rows_kernel, dim3(rgrid), dim3(256), 0, em->stream, R, em->base_count.p,
                                   em->plan.resample_cut, n_big.p, pass ? em->big_rows.p : (uint32_t *)nullptr);
                GBRS_HIP_CHECK(hipMemcpyAsync(&em->n_big, n_big.p, 4, hipMemcpyDeviceToHost, em->stream));
                GBRS_HIP_CHECK(hipStreamSynchronize(em->stream));
                if (em->n_big == 0) break;
                if (pass == 0) GBRS_TRY(em->big_rows.alloc(em->n_big));
            }
        } else {
            hipLaunchKernelGGL(resample_draw_kernel<true>, dim3(rgrid), dim3(256), 0, em->stream, R, (const uint32_t *)nullptr,
                               0u, 0u, 0u, 0u, em->count.p);
        }
        GBRS_HIP_CHECK(hipGetLastError());
    }
    if (eff_len) {
        GBRS_TRY(em->eff_len.alloc(LH));
        GBRS_HIP_CHECK(hipMemcpy(em->scratch_hl.p, eff_len, LH * sizeof(double), kind));
        hipLaunchKernelGGL(transpose_hl_to_lh, dim3(1024), dim3(256), 0, em->stream, L, H,
                           em->scratch_hl.p, em->eff_len.p);
        GBRS_HIP_CHECK(hipStreamSynchronize(em->stream));
    }
    GBRS_HIP_CHECK(hipDeviceSynchronize());
    GBRS_TRY(check_row_ids(n, em->ent_row.p, R, em->stream));
    stg.mark("vectors, checks");
    if ((flags & GBRS_EM_DETERMINISTIC) && !plan.tiled)
        return fail(GBRS_ERR_UNSUPPORTED, "GBRS_EM_DETERMINISTIC needs the tiled layout (H <= 16, not GBRS_EM_LAYOUT_CSC): "
                                          "the CSC kernels accumulate with global float atomics");
    if (plan.tiled) {
        em->tl.retain_temporaries = (flags & GBRS_EM_ONE_SHOT) != 0;
        em->tl.keep_row_ids = resample;
        GBRS_TRY(build_tile_layout(em->tl, R, n, em->ent_row.p, em->col_ptr.p, em->has_count ? em->count.p : nullptr, em->stream, plan));
        em->layout = 1;
        stg.mark("build_tile_layout");
        // the CSC copy and the per-row denominators are only needed by layout 0 (and, until
        // gbrs_em_set_initial_values has run, when the caller announced stored values)
        em->keep_csc = (flags & GBRS_EM_KEEP_CSC) != 0;
        // (models 1-3 build their layout from the row ids: GBRS_EM_GROUPED_MODELS keeps them; the posterior passes
        // walk them: GBRS_EM_POSTERIOR keeps them)
        const bool keep_rows = (flags & (GBRS_EM_GROUPED_MODELS | GBRS_EM_POSTERIOR)) != 0;
        if (!em->keep_csc) {
            if (em->tl.retain_temporaries) {  // one-shot process: left to the handle's destructor (common.h, DeferFrees)
                DeferFrees with_the_layout(&em->tl.retired, &em->tl.retired_bytes);
                if (!keep_rows) em->ent_row.release();
                em->den.release();
            } else {
                if (!keep_rows) em->ent_row.release();
                em->den.release();
            }
        }
        stg.mark("release csc copy");
    }
    guard.p = nullptr;
    *out = em;
    return GBRS_OK;
}

}  // namespace

struct gbrs_compress {
    int device = 0;
    uint32_t L = 0, H = 0;
    CompressResult res;
};

extern "C" {

int gbrs_compress_create(uint64_t R, uint32_t L, uint32_t H, const uint32_t *const *indptr,
                         const uint32_t *const *indices, const double *count, int device,
                         gbrs_compress_t **out, uint64_t *num_ecs, uint64_t *nnz_per_hap) {
    RoctxRange roctx_range("gbrs_compress_create");
    if (!out) return fail(GBRS_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (H < 1 || H > 16 || L < 1 || R < 1 || R > 0xFFFFFFFFull || !indptr || !indices)
        return fail(GBRS_ERR_INVALID, "The shape must be a tuple of three positive integers (H <= 16, R < 2^32).");
    GBRS_TRY(select_device(device));
    hipStream_t s = nullptr;
    GBRS_HIP_CHECK(hipStreamCreateWithFlags(&s, hipStreamDefault));
    struct SG { hipStream_t s; ~SG() { (void)hipStreamDestroy(s); } } sg{s};
    DevBuf<uint32_t> ent_row;
    DevBuf<uint64_t> col_ptr;
    DevBuf<double> d_count;
    uint64_t n = 0;
    GBRS_TRY(upload_csc(R, L, H, indptr, indices, false, ent_row, col_ptr, n));
    if (count) {
        GBRS_TRY(d_count.alloc(R));
        GBRS_HIP_CHECK(hipMemcpy(d_count.p, count, R * sizeof(double), hipMemcpyHostToDevice));
    }
    GBRS_HIP_CHECK(hipDeviceSynchronize());
    GBRS_TRY(check_row_ids(n, ent_row.p, R, s));
    gbrs_compress *c = new gbrs_compress();
    c->device = device; c->L = L; c->H = H;
    const int st = compress_device(c->res, R, L, H, n, ent_row.p, col_ptr.p, count ? d_count.p : nullptr, s);
    if (st != GBRS_OK) { delete c; return st; }
    if (num_ecs) *num_ecs = c->res.num_ecs;
    if (nnz_per_hap) {
        std::vector<uint64_t> cp((size_t)H * L + 1);
        GBRS_HIP_CHECK(hipMemcpy(cp.data(), c->res.col_ptr.p, cp.size() * 8, hipMemcpyDeviceToHost));
        for (uint32_t h = 0; h < H; ++h) nnz_per_hap[h] = cp[(size_t)(h + 1) * L] - cp[(size_t)h * L];
    }
    *out = c;
    return GBRS_OK;
}

int gbrs_compress_get(gbrs_compress_t *c, uint32_t *const *indptr_out, uint32_t *const *indices_out, double *count_out) {
    if (!c || !indptr_out || !indices_out) return fail(GBRS_ERR_INVALID, "NULL argument");
    GBRS_TRY(select_device(c->device));
    const uint32_t L = c->L, H = c->H;
    std::vector<uint64_t> cp((size_t)H * L + 1);
    GBRS_HIP_CHECK(hipMemcpy(cp.data(), c->res.col_ptr.p, cp.size() * 8, hipMemcpyDeviceToHost));
    for (uint32_t h = 0; h < H; ++h) {
        const uint64_t base = cp[(size_t)h * L], cnt = cp[(size_t)(h + 1) * L] - base;
        for (uint32_t l = 0; l <= L; ++l) indptr_out[h][l] = (uint32_t)(cp[(size_t)h * L + l] - base);
        if (cnt) GBRS_HIP_CHECK(hipMemcpy(indices_out[h], c->res.indices.p + base, cnt * 4, hipMemcpyDeviceToHost));
    }
    if (count_out && c->res.num_ecs)
        GBRS_HIP_CHECK(hipMemcpy(count_out, c->res.count.p, c->res.num_ecs * 8, hipMemcpyDeviceToHost));
    return GBRS_OK;
}

int gbrs_compress_destroy(gbrs_compress_t *c) {
    if (c) { (void)hipSetDevice(c->device); delete c; }
    return GBRS_OK;
}

}  // extern "C"

extern "C" {

int gbrs_em_create(uint64_t R, uint32_t L, uint32_t H, const uint32_t *const *indptr,
                   const uint32_t *const *indices, const double *count, const double *eff_len,
                   int device, uint32_t flags, gbrs_em_t **out) {
    return em_create_impl(R, L, H, indptr, indices, count, eff_len, nullptr, device, flags, false, out);
}

int gbrs_em_create_device(uint64_t R, uint32_t L, uint32_t H, const uint32_t *const *indptr,
                          const uint32_t *const *indices, const double *count, const double *eff_len,
                          int device, uint32_t flags, gbrs_em_t **out) {
    return em_create_impl(R, L, H, indptr, indices, count, eff_len, nullptr, device, flags, true, out);
}

int gbrs_em_create_masked(uint64_t R, uint32_t L, uint32_t H, const uint32_t *const *indptr,
                          const uint32_t *const *indices, const double *count, const double *eff_len,
                          const uint32_t *allowed, int device, uint32_t flags, gbrs_em_t **out) {
    if (allowed && H < 32)
        for (uint32_t l = 0; l < L; ++l)
            if (allowed[l] >> H) return fail(GBRS_ERR_INVALID, "allowed[%u] names a haplotype >= num_haps", l);
    return em_create_impl(R, L, H, indptr, indices, count, eff_len, allowed, device, flags, false, out);
}

int gbrs_em_create_masked_device(uint64_t R, uint32_t L, uint32_t H, const uint32_t *const *indptr,
                                 const uint32_t *const *indices, const double *count, const double *eff_len,
                                 const uint32_t *allowed, int device, uint32_t flags, gbrs_em_t **out) {
    if (allowed && H < 32)
        for (uint32_t l = 0; l < L; ++l)
            if (allowed[l] >> H) return fail(GBRS_ERR_INVALID, "allowed[%u] names a haplotype >= num_haps", l);
    return em_create_impl(R, L, H, indptr, indices, count, eff_len, allowed, device, flags, true, out);
}

namespace {
// partial sums of count/nnz_row into em->acc (every element written)
int em_prepare_partial(gbrs_em *em) {
    GBRS_TRY(select_device(em->device));
    GBRS_TRY(em_reset_scalars(em, false));
    em->post_model = 0;                       // no E-step since this prepare: nothing for gbrs_em_posterior
    if (em->has_init) {                       // stored alignment values: their normalised column sums
        GBRS_HIP_CHECK(hipMemcpyAsync(em->acc.p, em->acc_init.p, em->acc.bytes(), hipMemcpyDeviceToDevice, em->stream));
        return GBRS_OK;
    }
    return em_estep(em, em_route(em, EmPass::Prepare));
}
}  // namespace

int gbrs_em_set_initial_values(gbrs_em_t *em, const double *const *values) {
    if (!em || !values) return fail(GBRS_ERR_INVALID, "NULL argument");
    if (em->resample)
        return fail(GBRS_ERR_UNSUPPORTED, "stored alignment values are not available on a GBRS_EM_RESAMPLE handle: their "
                                          "cached column sums would carry the count they were made with");
    if (!em->ent_row.p || !em->den.p)
        return fail(GBRS_ERR_STATE, "the handle no longer holds the CSC arrays: create it with GBRS_EM_KEEP_CSC "
                                    "and call gbrs_em_set_initial_values once, before prepare");
    GBRS_TRY(select_device(em->device));
    const uint64_t n = em->N;
    const size_t LH = (size_t)em->L * em->H;
    GBRS_TRY(em->acc_init.alloc(LH));
    GBRS_HIP_CHECK(hipMemsetAsync(em->acc_init.p, 0, em->acc_init.bytes(), em->stream));
    if (n) {
        DevBuf<double> vals;
        DevBuf<int> bad;
        GBRS_TRY(vals.alloc(n));
        GBRS_TRY(bad.alloc(1));
        // values[h] lines up with indices[h] as given to create: under a haplotype mask they are staged whole and
        // then moved the way the row ids were (compact_columns_kernel)
        const DevBuf<uint64_t> &given = em->masked ? em->col_ptr_src : em->col_ptr;
        if (!given.p) return fail(GBRS_ERR_STATE, "the handle no longer knows the layout of the caller's arrays");
        std::vector<uint64_t> cp((size_t)em->H * em->L + 1);
        GBRS_HIP_CHECK(hipMemcpy(cp.data(), given.p, cp.size() * 8, hipMemcpyDeviceToHost));
        DevBuf<double> staged;
        if (em->masked) GBRS_TRY(staged.alloc(std::max<uint64_t>(cp.back(), 1)));
        double *dst = em->masked ? staged.p : vals.p;
        for (uint32_t h = 0; h < em->H; ++h) {
            const uint64_t b = cp[(size_t)h * em->L], cnt = cp[(size_t)(h + 1) * em->L] - b;
            if (!cnt) continue;
            if (!values[h]) return fail(GBRS_ERR_INVALID, "values[%u] is NULL", h);
            GBRS_HIP_CHECK(hipMemcpy(dst + b, values[h], cnt * sizeof(double), hipMemcpyHostToDevice));
        }
        if (em->masked) {
            hipLaunchKernelGGL(compact_columns_kernel<double>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, em->stream,
                               n, em->H * em->L, em->col_ptr.p, em->col_ptr_src.p, staged.p, vals.p);
            GBRS_HIP_CHECK(hipStreamSynchronize(em->stream));
        }
        GBRS_HIP_CHECK(hipMemsetAsync(bad.p, 0, sizeof(int), em->stream));
        GBRS_HIP_CHECK(hipMemsetAsync(em->den.p, 0, em->den.bytes(), em->stream));
        const unsigned grid = (unsigned)((n + 255) / 256);
        hipLaunchKernelGGL(csc_den_values_kernel, dim3(grid), dim3(256), 0, em->stream, n, em->ent_row.p, vals.p, em->den.p);
        hipLaunchKernelGGL(csc_acc_values_kernel, dim3(grid), dim3(256), 0, em->stream, n, em->H * em->L, em->L, em->H,
                           em->col_ptr.p, em->ent_row.p, vals.p, em->has_count ? em->count.p : (const double *)nullptr,
                           em->den.p, em->acc_init.p, bad.p);
        int hbad = 0;
        GBRS_HIP_CHECK(hipMemcpyAsync(&hbad, bad.p, sizeof(int), hipMemcpyDeviceToHost, em->stream));
        GBRS_HIP_CHECK(hipStreamSynchronize(em->stream));
        GBRS_HIP_CHECK(hipGetLastError());
        if (hbad) {
            em->acc_init.release();
            return fail(GBRS_ERR_FLOAT, "invalid value encountered in divide (a read's stored alignment values are "
                                        "negative or add up to zero)");
        }
    }
    em->has_init = true;
    if (em->layout == 1 && em->keep_csc) {     // the tiled layout needs neither array from here on
        if (!(em->flags & (GBRS_EM_GROUPED_MODELS | GBRS_EM_POSTERIOR))) em->ent_row.release();
        em->den.release();
        em->col_ptr_src.release();
        em->keep_csc = false;
    }
    return GBRS_OK;
}

int gbrs_em_prepare_partial(gbrs_em_t *em, void **partial_dev, uint64_t *n_elems) {
    if (!em) return fail(GBRS_ERR_INVALID, "handle is NULL");
    em->acc_external = true;                  // sharded rows: the caller all-reduces the whole A vector from now on
    GBRS_TRY(em_prepare_partial(em));
    if (partial_dev) *partial_dev = em->acc.p;
    if (n_elems) *n_elems = (uint64_t)em->L * em->H;
    return GBRS_OK;
}

int gbrs_em_finish_prepare(gbrs_em_t *em, double pseudocount) {
    if (!em) return fail(GBRS_ERR_INVALID, "handle is NULL");
    GBRS_TRY(select_device(em->device));
    GBRS_TRY(em_finish_prepare(em, pseudocount));
    EmScalars host;
    return em_check_float(em, host);
}

int gbrs_em_prepare(gbrs_em_t *em, double pseudocount) {
    RoctxRange roctx_range("gbrs_em_prepare");
    if (!em) return fail(GBRS_ERR_INVALID, "handle is NULL");
    GBRS_TRY(em_prepare_partial(em));
    return gbrs_em_finish_prepare(em, pseudocount);
}

int gbrs_em_estep_partial(gbrs_em_t *em, void **partial_dev, uint64_t *n_elems) {
    if (!em) return fail(GBRS_ERR_INVALID, "handle is NULL");
    if (!em->prepared) return fail(GBRS_ERR_STATE, "prepare() has not been called");
    GBRS_TRY(select_device(em->device));
    // a run that met its stopping rule (gbrs_em_run, or the pair's rule: gbrs_em_pair_check) left the device's stop flag
    // set, which turns every step kernel into a no-op; a step asked for by hand is applied anyway, as in gbrs_em_step
    if (em->stopped) GBRS_TRY(em_reset_scalars(em, true));
    em->acc_external = true;                  // acc is handed out: every route of the handle gathers all of it from here on
    GBRS_TRY(em_estep(em, em_route(em, EmPass::Partial)));
    if (partial_dev) *partial_dev = em->acc.p;
    if (n_elems) *n_elems = (uint64_t)em->L * em->H;
    return GBRS_OK;
}

int gbrs_em_finish_step(gbrs_em_t *em, double *err_sum_out) {
    if (!em) return fail(GBRS_ERR_INVALID, "handle is NULL");
    GBRS_TRY(select_device(em->device));
    // without a request for err_sum the error pass is deferred into the next E-step launch
    GBRS_TRY(em_finish_step(em, em_route(em, EmPass::Partial), -1.0, /* defer_err */ err_sum_out == nullptr));
    if (em->pair_ev_mstep) GBRS_HIP_CHECK(hipEventRecord(em->pair_ev_mstep, em->stream));
    if (err_sum_out) {
        EmScalars host;
        GBRS_TRY(em_check_float(em, host));
        *err_sum_out = host.err_sum;
    }
    return GBRS_OK;
}

int gbrs_em_step(gbrs_em_t *em, int n_iters, double *err_sum_out) {
    RoctxRange roctx_range("gbrs_em_step");
    if (!em) return fail(GBRS_ERR_INVALID, "handle is NULL");
    if (!em->prepared) return fail(GBRS_ERR_STATE, "prepare() has not been called");
    GBRS_TRY(select_device(em->device));
    // a run that met its stopping rule left the device's stop flag set; a step asked for by hand is applied anyway
    // (EMfactory.update_allelic_expression knows no stopping rule)
    if (em->stopped) GBRS_TRY(em_reset_scalars(em, true));
    // (and at most EM_TIME_SAMPLES of them, spread over the call, the first iteration included: 500 iterations timed on
    // every eighth paid ~1.5 us each for the records)
    const int stride = std::max(EM_TIME_STRIDE, (n_iters + EM_TIME_SAMPLES - 1) / EM_TIME_SAMPLES);
    const int timed = em->time_steps ? (n_iters + stride - 1) / stride : 0;
    while ((int)em->ev_pool.size() < 3 * timed) {
        hipEvent_t e;
        GBRS_HIP_CHECK(hipEventCreate(&e));
        em->ev_pool.push_back(e);
    }
    const EmStepRoute route = em_route(em, EmPass::Step);
    if (em_gather_route(em) && n_iters > 0) {
        // the gather-side M-step (em_gather_steps); the first M-step since theta was set runs on the route above, once: the
        // loci without reads still carry theta there, and count in that iteration's totals
        int left = n_iters;
        if (!em->gm.primed) {
            GBRS_TRY(em_one_step(em, route, 4, -1.0, left == 1 ? em->ev_pool.data() : nullptr, false));
            --left;
        }
        const int gtimed = left == 0 ? 1 : std::min(timed, (left + stride - 1) / stride);
        if (left > 0) GBRS_TRY(em_gather_steps(em, left, -1.0, stride, gtimed));
        EmScalars host;
        std::memset(&host, 0, sizeof(host));
        const int float_rc = em_check_float(em, host);
        // (only a NaN error sum stops a step asked for by hand, and a float error comes with it: the next call starts over
        // on the plain route, from whatever theta the caller sets)
        if (host.stop || float_rc != GBRS_OK) em->gm.clean = em->gm.primed = false;
        GBRS_TRY(float_rc);
        em_read_times(em, gtimed);
        if (err_sum_out) *err_sum_out = host.err_sum;
        return GBRS_OK;
    }
    for (int i = 0; i < n_iters; ++i) {
        const int slot = i / stride;
        const bool t = i % stride == 0 && slot < timed;
        GBRS_TRY(em_one_step(em, route, 4, -1.0, t ? &em->ev_pool[3 * slot] : nullptr, i + 1 < n_iters));
    }
    EmScalars host;
    GBRS_TRY(em_check_float(em, host));
    em_read_times(em, timed);
    if (err_sum_out) *err_sum_out = host.err_sum;
    return GBRS_OK;
}

int gbrs_em_step_model(gbrs_em_t *em, int model, int n_iters, double *err_sum_out) {
    RoctxRange roctx_range("gbrs_em_step_model");
    if (!em) return fail(GBRS_ERR_INVALID, "handle is NULL");
    GBRS_TRY(em_check_model(em, model));
    if (model == 4) return gbrs_em_step(em, n_iters, err_sum_out);
    if (!em->prepared) return fail(GBRS_ERR_STATE, "prepare() has not been called");
    GBRS_TRY(select_device(em->device));
    if (em->stopped) GBRS_TRY(em_reset_scalars(em, true));     // as gbrs_em_step: a step asked for is applied
    GBRS_TRY(em_ensure_order(em, model));
    const EmStepRoute route = em_route(em, EmPass::Model);
    for (int i = 0; i < n_iters; ++i) GBRS_TRY(em_one_step(em, route, model, -1.0, i == 0 ? em->ev_pool.data() : nullptr, false));
    EmScalars host;
    GBRS_TRY(em_check_float(em, host));
    em_read_times(em, n_iters > 0 ? 1 : 0);
    if (err_sum_out) *err_sum_out = host.err_sum;
    return GBRS_OK;
}

int gbrs_em_set_groups(gbrs_em_t *em, int64_t G, const int64_t *group_ptr, const int64_t *members) {
    RoctxRange roctx_range("gbrs_em_set_groups");
    if (!em || G < 0 || (G > 0 && (!group_ptr || !members))) return fail(GBRS_ERR_INVALID, "bad argument");
    if (!(em->flags & GBRS_EM_GROUPED_MODELS))
        return fail(GBRS_ERR_STATE, "the handle was not created with GBRS_EM_GROUPED_MODELS");
    if (em->N && !em->ent_row.p) return fail(GBRS_ERR_STATE, "the handle no longer holds the CSC row ids");
    const uint32_t L = em->L, H = em->H;
    if (em->N >= 0xFFFFFFFFull || L >= (1u << 27))
        return fail(GBRS_ERR_UNSUPPORTED, "the grouped layout holds at most 2^32 - 1 entries of at most 2^27 loci");
    if (G > 0 && group_ptr[0] != 0) return fail(GBRS_ERR_INVALID, "group_ptr[0] != 0");
    for (int64_t g = 0; g < G; ++g)
        if (group_ptr[g + 1] < group_ptr[g]) return fail(GBRS_ERR_INVALID, "group_ptr not monotone");
    GBRS_TRY(select_device(em->device));
    // genes: the groups in order (members ascending, a repeat inside a group counted once), then every locus in no
    // group as a gene of its own, in locus order
    std::vector<int64_t> gene(L, -1);
    std::vector<std::vector<uint32_t>> mem((size_t)G);
    for (int64_t g = 0; g < G; ++g)
        for (int64_t k = group_ptr[g]; k < group_ptr[g + 1]; ++k) {
            const int64_t l = members[k];
            if (l < 0 || l >= (int64_t)L) return fail(GBRS_ERR_INVALID, "group member %lld out of range", (long long)l);
            if (gene[l] == g) continue;
            if (gene[l] >= 0)
                return fail(GBRS_ERR_INVALID, "locus %lld is in two groups (%lld and %lld)", (long long)l,
                            (long long)gene[l], (long long)g);
            gene[l] = g;
            mem[g].push_back((uint32_t)l);
        }
    std::vector<uint32_t> gptr{0}, gmem, lgene(L), pos(L);
    gmem.reserve(L);
    for (int64_t g = 0; g < G; ++g) {
        std::sort(mem[g].begin(), mem[g].end());
        for (uint32_t l : mem[g]) { lgene[l] = (uint32_t)(gptr.size() - 1); pos[l] = (uint32_t)gmem.size(); gmem.push_back(l); }
        gptr.push_back((uint32_t)gmem.size());
    }
    for (uint32_t l = 0; l < L; ++l)
        if (gene[l] < 0) { lgene[l] = (uint32_t)(gptr.size() - 1); pos[l] = (uint32_t)gmem.size(); gmem.push_back(l); gptr.push_back((uint32_t)gmem.size()); }
    const uint32_t n_genes = (uint32_t)(gptr.size() - 1);
    // sort ranks of the columns: (gene, locus, haplotype) = pos*H + h; (gene, haplotype, locus) inside the gene's block
    const size_t HL = (size_t)H * L;
    std::vector<uint32_t> r23(HL), i23(HL), r1(HL), i1(HL);
    for (uint32_t l = 0; l < L; ++l) {
        const uint32_t g = lgene[l], start = gptr[g], size = gptr[g + 1] - start;
        for (uint32_t h = 0; h < H; ++h) {
            const uint32_t a = pos[l] * H + h, b = start * H + h * size + (pos[l] - start);
            r23[(size_t)h * L + l] = a;
            i23[a] = l * 32u + h;
            r1[(size_t)h * L + l] = b;
            i1[b] = l * 32u + h;
        }
    }
    em->grouped = false;
    em->order_m1.built = em->order_m23.built = false;
    auto up = [&](DevBuf<uint32_t> &d, const std::vector<uint32_t> &v) -> int {
        GBRS_TRY(d.alloc(std::max<size_t>(v.size(), 1)));
        if (!v.empty()) GBRS_HIP_CHECK(hipMemcpyAsync(d.p, v.data(), v.size() * 4, hipMemcpyHostToDevice, em->stream));
        return GBRS_OK;
    };
    GBRS_TRY(up(em->gene_ptr, gptr));
    GBRS_TRY(up(em->gene_mem, gmem));
    GBRS_TRY(up(em->locus_gene, lgene));
    GBRS_TRY(up(em->rank_m23, r23));
    GBRS_TRY(up(em->inv_m23, i23));
    GBRS_TRY(up(em->rank_m1, r1));
    GBRS_TRY(up(em->inv_m1, i1));
    GBRS_TRY(em->gene_tot.alloc(n_genes));
    GBRS_TRY(em->gene_hap_tot.alloc((size_t)n_genes * H));
    GBRS_TRY(em->locus_tot.alloc(L));
    GBRS_TRY(em->fac.alloc(std::max<uint64_t>(em->N, 1)));
    GBRS_HIP_CHECK(hipStreamSynchronize(em->stream));       // (the host vectors go out of scope)
    em->n_genes = n_genes;
    GBRS_TRY(build_row_ptr(em->row_ptr, em->R, em->N, em->ent_row.p, em->stream));
    GBRS_TRY(build_grouped_order(em->order_m23, em->R, L, H, em->N, em->ent_row.p, em->col_ptr.p, em->rank_m23.p,
                                 em->inv_m23.p, em->stream));
    em->grouped = true;
    return GBRS_OK;
}

int gbrs_em_run(gbrs_em_t *em, int model, double tol, int max_iters, int *n_iters_out,
                double *err_hist, int err_hist_cap, double *elapsed_s) {
    RoctxRange roctx_range("gbrs_em_run");
    if (!em) return fail(GBRS_ERR_INVALID, "handle is NULL");
    GBRS_TRY(em_check_model(em, model));
    if (!em->prepared) return fail(GBRS_ERR_STATE, "prepare() has not been called");
    GBRS_TRY(select_device(em->device));
    if (model != 4) GBRS_TRY(em_ensure_order(em, model));
    if (max_iters < 0) max_iters = 0;
    GBRS_TRY(em_ensure_hist(em, std::max(max_iters, 1)));
    GBRS_TRY(em_reset_scalars(em, false));
    const double target = 1000000.0 * tol;
    const EmStepRoute route = em_route(em, model == 4 ? EmPass::Step : EmPass::Model);
    // the reference tests `err_sum > target` with err_sum = 1e6 before the first step
    int done = 0;
    EmScalars host;
    std::memset(&host, 0, sizeof(host));
    if (1000000.0 > target) {
        // Steps are enqueued in batches of 8 (one host synchronisation each); a device-side stop flag
        // turns the steps after the stopping iteration into no-ops, so theta is exactly the stopping
        // iteration's value.
        const int batch = 8;
        bool first = true;
        const auto t_start = std::chrono::steady_clock::now();
        while (done < max_iters) {
            const int nb = std::min(batch, max_iters - done);
            // (the gather-side M-step, em_gather_steps: the first M-step since theta was set on the route above, once)
            const bool gather = model == 4 && em_gather_route(em);
            int left = nb;
            if (gather && !em->gm.primed) {
                GBRS_TRY(em_one_step(em, route, model, target, first ? em->ev_pool.data() : nullptr, false));
                first = false;
                --left;
            }
            const int gk = gather ? left : 0, g_it0 = done + (nb - left);
            if (gk > 0) {
                // (a stop raised by the step above turns every launch of this call into a no-op)
                GBRS_TRY(em_gather_steps(em, gk, target, gk, first ? 1 : 0));
                first = false;
                left = 0;
            }
            for (int i = 0; i < left; ++i) {     // the run's first step is timed; a batch's last error pass is not deferred
                GBRS_TRY(em_one_step(em, route, model, target, first ? em->ev_pool.data() : nullptr, i + 1 < nb));
                first = false;
            }
            // (a float error is reported after the handle is settled: a stop raised with it must not leave the half-written
            // theta vector current)
            const int float_rc = em_check_float(em, host);
            if (gk > 0 && host.stop) em_gather_settle(em, g_it0, host.iters_done);
            GBRS_TRY(float_rc);
            if (elapsed_s) {       // the host sees a batch at a time: its iterations share the batch's completion time
                const double t = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count();
                for (int i = done; i < host.iters_done && i < err_hist_cap; ++i) elapsed_s[i] = t;
            }
            done = host.iters_done;
            if (host.stop) break;
        }
    }
    em_read_times(em, 1);
    if (n_iters_out) *n_iters_out = done;
    if (err_hist && err_hist_cap > 0 && done > 0) {
        const int ncopy = std::min(done, err_hist_cap);
        GBRS_HIP_CHECK(hipMemcpy(err_hist, em->err_hist.p, ncopy * sizeof(double), hipMemcpyDeviceToHost));
    }
    return GBRS_OK;
}

int gbrs_em_get(gbrs_em_t *em, double *theta, double *expected_counts) {
    if (!em) return fail(GBRS_ERR_INVALID, "handle is NULL");
    GBRS_TRY(select_device(em->device));
    const size_t LH = (size_t)em->L * em->H;
    for (int which = 0; which < 2; ++which) {
        double *dst = which == 0 ? theta : expected_counts;
        if (!dst) continue;
        if (which == 1) GBRS_TRY(em_refresh_counts(em));
        hipLaunchKernelGGL(transpose_lh_to_hl, dim3(1024), dim3(256), 0, em->stream, em->L, em->H,
                           which == 0 ? em->theta.p : em->counts.p, em->scratch_hl.p);
        GBRS_HIP_CHECK(hipMemcpyAsync(dst, em->scratch_hl.p, LH * sizeof(double), hipMemcpyDeviceToHost, em->stream));
        GBRS_HIP_CHECK(hipStreamSynchronize(em->stream));
    }
    return GBRS_OK;
}

int gbrs_em_posterior(gbrs_em_t *em, uint32_t hap, double *out, uint64_t out_len) {
    RoctxRange roctx_range("gbrs_em_posterior");
    if (!em) return fail(GBRS_ERR_INVALID, "handle is NULL");
    if (!(em->flags & GBRS_EM_POSTERIOR))
        return fail(GBRS_ERR_STATE, "the handle was not created with GBRS_EM_POSTERIOR");
    if (em->post_model == 0) return fail(GBRS_ERR_STATE, "no EM step has run since prepare: there is no posterior yet");
    if (hap >= em->H) return fail(GBRS_ERR_INVALID, "haplotype %u >= num_haps %u", hap, em->H);
    GBRS_TRY(select_device(em->device));
    GBRS_TRY(em_flush_err(em));
    const uint32_t L = em->L, H = em->H, ncols = H * L;
    uint64_t k0 = 0, k1 = 0;                   // the haplotype's columns are one piece of the concatenated arrays
    GBRS_HIP_CHECK(hipMemcpyAsync(&k0, em->col_ptr.p + (size_t)hap * L, sizeof(k0), hipMemcpyDeviceToHost, em->stream));
    GBRS_HIP_CHECK(hipMemcpyAsync(&k1, em->col_ptr.p + (size_t)(hap + 1) * L, sizeof(k1), hipMemcpyDeviceToHost, em->stream));
    GBRS_HIP_CHECK(hipStreamSynchronize(em->stream));
    if (k1 < k0 || k1 > em->N) return fail(GBRS_ERR_STATE, "the kept column pointers are damaged");
    const uint64_t n_h = k1 - k0;
    if (out_len != n_h)
        return fail(GBRS_ERR_INVALID, "out_len is %llu, haplotype %u has %llu stored entries", (unsigned long long)out_len,
                    hap, (unsigned long long)n_h);
    if (n_h == 0) return GBRS_OK;
    if (!out) return fail(GBRS_ERR_INVALID, "out is NULL");
    if (!em->ent_row.p) return fail(GBRS_ERR_STATE, "the handle no longer holds the CSC row ids");
    const bool model4 = em->post_model == 4;
    if (!model4 && !em->fac.p) return fail(GBRS_ERR_STATE, "the handle holds no factors of a model %d step", em->post_model);
    if (model4 && !em->post_den_valid) {       // once per step, shared by the calls for the H haplotypes
        GBRS_HIP_CHECK(hipMemsetAsync(em->post_den.p, 0, em->post_den.bytes(), em->stream));
        hipLaunchKernelGGL(post_den_kernel, dim3((unsigned)((em->N + 255) / 256)), dim3(256), 0, em->stream, em->N, ncols,
                           L, H, em->col_ptr.p, em->ent_row.p, em->theta_kept.p, em->post_den.p);
        GBRS_HIP_CHECK(hipGetLastError());
        em->post_den_valid = true;
    }
    if (em->post_vals.n < n_h) {               // one haplotype's values at a time: sized for the longest one
        std::vector<uint64_t> cp((size_t)ncols + 1);
        GBRS_HIP_CHECK(hipMemcpy(cp.data(), em->col_ptr.p, cp.size() * 8, hipMemcpyDeviceToHost));
        uint64_t longest = 0;
        for (uint32_t h = 0; h < H; ++h) longest = std::max(longest, cp[(size_t)(h + 1) * L] - cp[(size_t)h * L]);
        GBRS_HIP_CHECK(hipStreamSynchronize(em->stream));
        GBRS_TRY(em->post_vals.alloc(longest));
    }
    const dim3 grid((unsigned)((n_h + 255) / 256));
    const double *cnt = em->has_count ? em->count.p : (const double *)nullptr;
    if (model4)
        hipLaunchKernelGGL(post_value_kernel<true>, grid, dim3(256), 0, em->stream, k0, k1, ncols, L, H, hap, em->col_ptr.p,
                           em->ent_row.p, em->theta_kept.p, em->post_den.p, (const double *)nullptr, cnt, em->post_vals.p);
    else
        hipLaunchKernelGGL(post_value_kernel<false>, grid, dim3(256), 0, em->stream, k0, k1, ncols, L, H, hap, em->col_ptr.p,
                           em->ent_row.p, em->theta_kept.p, (const double *)nullptr, em->fac.p, cnt, em->post_vals.p);
    GBRS_HIP_CHECK(hipGetLastError());
    GBRS_HIP_CHECK(hipMemcpyAsync(out, em->post_vals.p, n_h * sizeof(double), hipMemcpyDeviceToHost, em->stream));
    GBRS_HIP_CHECK(hipStreamSynchronize(em->stream));
    return GBRS_OK;
}

int gbrs_em_set_theta(gbrs_em_t *em, const double *theta) {
    if (!em || !theta) return fail(GBRS_ERR_INVALID, "NULL argument");
    GBRS_TRY(select_device(em->device));
    const size_t LH = (size_t)em->L * em->H;
    // the expected counts stay those of the last iteration (the reports rescale theta to TPM in place and then ask for
    // the counts, EMfactory.py:352-354 before :302): made from the theta about to be replaced, if not stored yet
    GBRS_TRY(em_refresh_counts(em));
    GBRS_HIP_CHECK(hipMemcpyAsync(em->scratch_hl.p, theta, LH * sizeof(double), hipMemcpyHostToDevice, em->stream));
    hipLaunchKernelGGL(transpose_hl_to_lh, dim3(1024), dim3(256), 0, em->stream, em->L, em->H,
                       em->scratch_hl.p, em->theta.p);
    GBRS_HIP_CHECK(hipStreamSynchronize(em->stream));
    em->prepared = true;
    em->gm.primed = false;
    return GBRS_OK;
}

int gbrs_em_group_sums(gbrs_em_t *em, int64_t G, const int64_t *group_ptr, const int64_t *members,
                       int which, double *out) {
    if (!em || !group_ptr || !out || G < 0) return fail(GBRS_ERR_INVALID, "bad argument");
    if (G == 0) return GBRS_OK;
    GBRS_TRY(select_device(em->device));
    const int64_t nm = group_ptr[G];
    for (int64_t g = 0; g < G; ++g)
        if (group_ptr[g + 1] < group_ptr[g]) return fail(GBRS_ERR_INVALID, "group_ptr not monotone");
    for (int64_t k = 0; k < nm; ++k)
        if (members[k] < 0 || members[k] >= (int64_t)em->L)
            return fail(GBRS_ERR_INVALID, "group member %lld out of range", (long long)members[k]);
    DevBuf<int64_t> d_ptr, d_mem;
    DevBuf<double> d_out;
    GBRS_TRY(d_ptr.alloc(G + 1));
    GBRS_TRY(d_mem.alloc(std::max<int64_t>(nm, 1)));
    GBRS_TRY(d_out.alloc((size_t)G * em->H));
    GBRS_HIP_CHECK(hipMemcpyAsync(d_ptr.p, group_ptr, (G + 1) * sizeof(int64_t), hipMemcpyHostToDevice, em->stream));
    if (nm) GBRS_HIP_CHECK(hipMemcpyAsync(d_mem.p, members, nm * sizeof(int64_t), hipMemcpyHostToDevice, em->stream));
    const int64_t total = G * (int64_t)em->H;
    if (which != 0) GBRS_TRY(em_refresh_counts(em));
    hipLaunchKernelGGL(group_sum_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, em->stream,
                       em->H, G, d_ptr.p, d_mem.p, which == 0 ? em->theta.p : em->counts.p, d_out.p);
    GBRS_HIP_CHECK(hipMemcpyAsync(out, d_out.p, (size_t)G * em->H * sizeof(double), hipMemcpyDeviceToHost, em->stream));
    GBRS_HIP_CHECK(hipStreamSynchronize(em->stream));
    return GBRS_OK;
}

void *gbrs_em_stream(gbrs_em_t *em) { return em ? (void *)em->stream : nullptr; }

#if defined(GBRS_DIAG_TILE_TIMES)
// diagnostic build only: device buffer of 8 x uint64 per E-step workgroup (nullptr switches the stamps off)
int gbrs_debug_set_tile_stamps(void *device_ptr) {
    unsigned long long *p = static_cast<unsigned long long *>(device_ptr);
    GBRS_HIP_CHECK(hipMemcpyToSymbol(HIP_SYMBOL(g_tile_stamps), &p, sizeof(p)));
    return GBRS_OK;
}
#endif

int gbrs_em_set_stream(gbrs_em_t *em, void *stream) {
    if (!em) return fail(GBRS_ERR_INVALID, "handle is NULL");
    GBRS_TRY(select_device(em->device));
    GBRS_HIP_CHECK(hipStreamSynchronize(em->stream));
    if (em->own_stream && em->stream) (void)hipStreamDestroy(em->stream);
    em->stream = (hipStream_t)stream;
    em->own_stream = false;
    return GBRS_OK;
}

int gbrs_em_sync(gbrs_em_t *em) {
    if (!em) return fail(GBRS_ERR_INVALID, "handle is NULL");
    GBRS_TRY(em_flush_err(em));
    GBRS_HIP_CHECK(hipStreamSynchronize(em->stream));
    return GBRS_OK;
}

int gbrs_em_pair_begin(gbrs_em_t *a, gbrs_em_t *b, int max_iters) {
    if (!a || !b || a == b) return fail(GBRS_ERR_INVALID, "two distinct handles are needed");
    if (a->device != b->device) return fail(GBRS_ERR_INVALID, "the two handles of a pair live on one device");
    GBRS_TRY(select_device(a->device));
    for (gbrs_em *em : {a, b}) {
        GBRS_TRY(em_reset_scalars(em, false));           // (synchronises the handle's stream)
        if (!em->pair_ev_mstep) GBRS_HIP_CHECK(hipEventCreateWithFlags(&em->pair_ev_mstep, hipEventDisableTiming));
    }
    if (!a->pair_ev_err) GBRS_HIP_CHECK(hipEventCreateWithFlags(&a->pair_ev_err, hipEventDisableTiming));
    const int cap = std::max(max_iters, 1);
    if (!a->pair_sc.p) GBRS_TRY(a->pair_sc.alloc(1));
    if (cap > a->pair_hist_cap) {
        GBRS_TRY(a->pair_hist.alloc((size_t)cap));
        a->pair_hist_cap = cap;
    }
    GBRS_HIP_CHECK(hipMemset(a->pair_sc.p, 0, sizeof(gbrs_em::PairScalars)));
    return GBRS_OK;
}

int gbrs_em_pair_check(gbrs_em_t *a, gbrs_em_t *b, double tol) {
    if (!a || !b || !a->pair_sc.p || !a->pair_ev_err || !a->pair_ev_mstep || !b->pair_ev_mstep)
        return fail(GBRS_ERR_STATE, "gbrs_em_pair_begin has not been called on this pair");
    GBRS_TRY(select_device(a->device));
    // on b's stream (whose M-step has just been enqueued), after a's M-step; a's next M-step waits for the verdict
    GBRS_HIP_CHECK(hipStreamWaitEvent(b->stream, a->pair_ev_mstep, 0));
    static_assert(sizeof(PairState) == sizeof(gbrs_em::PairScalars), "one struct, two names");
    const PairSide sa{a->L, (int)a->msum_blocks, a->msum_cap, a->tot_prev.p, a->tot_new.p, a->msums.p, a->scalars.p};
    const PairSide sb{b->L, (int)b->msum_blocks, b->msum_cap, b->tot_prev.p, b->tot_new.p, b->msums.p, b->scalars.p};
    hipLaunchKernelGGL(pair_err_kernel, dim3(1), dim3(1024), 0, b->stream, sa, sb, 1000000.0 * tol,
                       reinterpret_cast<PairState *>(a->pair_sc.p), a->pair_hist.p, a->pair_hist_cap);
    GBRS_HIP_CHECK(hipGetLastError());
    GBRS_HIP_CHECK(hipEventRecord(a->pair_ev_err, b->stream));
    GBRS_HIP_CHECK(hipStreamWaitEvent(a->stream, a->pair_ev_err, 0));
    return GBRS_OK;
}

int gbrs_em_pair_status(gbrs_em_t *a, gbrs_em_t *b, int *iters_done, int *stopped, double *err_hist, int err_hist_cap) {
    if (!a || !b || !a->pair_sc.p) return fail(GBRS_ERR_STATE, "gbrs_em_pair_begin has not been called on this pair");
    GBRS_TRY(select_device(a->device));
    EmScalars ha, hb;
    GBRS_TRY(em_check_float(a, ha));                     // flushes deferred passes, synchronises, reports 0/0
    GBRS_TRY(em_check_float(b, hb));
    gbrs_em::PairScalars ps;
    GBRS_HIP_CHECK(hipMemcpy(&ps, a->pair_sc.p, sizeof(ps), hipMemcpyDeviceToHost));
    if (iters_done) *iters_done = ps.iters;
    if (stopped) *stopped = ps.stop;
    if (err_hist && err_hist_cap > 0 && ps.iters > 0)
        GBRS_HIP_CHECK(hipMemcpy(err_hist, a->pair_hist.p, std::min(ps.iters, std::min(err_hist_cap, a->pair_hist_cap)) * sizeof(double),
                                 hipMemcpyDeviceToHost));
    return GBRS_OK;
}

int gbrs_em_info(gbrs_em_t *em, gbrs_em_info_t *info) {
    if (!em || !info) return fail(GBRS_ERR_INVALID, "NULL argument");
    std::memset(info, 0, sizeof(*info));
    const uint64_t HL = (uint64_t)em->H * em->L;
    info->num_rows = em->R;
    info->num_entries = em->N;
    info->num_device_rows = em->R;
    info->num_device_words = em->N;
    info->algorithmic_bytes = 4 * em->N + 4 * (em->R + 1) + (em->has_count ? 8 * em->R : 0) +
                              16 * HL + (em->has_len ? 8 * HL : 0);
    // layout 0: two passes over the row ids + den zero/atomic/read + theta/acc traffic
    info->bytes_per_iter = 8 * em->N + 8 * em->R * 3 + 8 * HL * 4;
    info->estep_bytes = 8 * em->N + 8 * em->R * 3 + 8 * HL * 2;
    if (em->layout == 1) {
        const TileLayout &tl = em->tl;
        info->num_device_rows = tl.n_rows + tl.n_folded + tl.n_folded_two + tl.n_long;     // every read the layout represents
        info->num_folded_rows = (uint32_t)tl.n_folded;
        info->num_tiles = tl.n_tiles;
        info->num_slots = tl.n_slots;
        info->num_long_rows = tl.n_long;
        info->num_device_words = tl.n_batches * 64;
        // E-step: word stream, tile headers, dictionary, theta gather + partial store per slot,
        // [row weights]; gather: slot index + partials read back + acc store; M-step etc.: 5 H*L vectors
        // rows = theta rows gathered and sum rows stored by the tiles: one per slot, one per (slot, member) for a locus set
        const uint64_t rows = tl.n_dest_rows ? tl.n_dest_rows : tl.n_slots;
        info->bytes_per_iter = 4 * tl.n_batches * 64 + 16 * tl.n_tiles + 4 * tl.n_slots +
                               8 * rows * em->plan.tH * 3 + 4 * rows + 4 * ((uint64_t)em->plan.tL + 1) +
                               (tl.weighted ? 8 * tl.n_batches * 64 : 0) + 8 * HL * 6;
        info->num_heavy_loci = tl.n_heavy;
        info->num_light_loci = tl.n_light;
        // the E-step launch alone: words, tile headers, dictionary + slot destinations, theta gathered
        // once per slot, one partial-sum row stored per slot [, the per-word row weights]
        info->estep_bytes = 4 * tl.n_batches * 64 + 16 * tl.n_tiles + 4 * tl.n_slots + 4 * rows +
                            8 * rows * em->plan.tH * 2 + (tl.weighted ? 8 * tl.n_batches * 64 : 0) +
                            (tl.n_sets ? 8 * tl.n_slots : 0);       // dict_b / dest_b beside the dictionary
        if (tl.n_sets) info->bytes_per_iter += 8 * tl.n_slots;
        if (em_gather_route(em)) {
            // the gather-side route, one launch per iteration: words, headers, dictionary + the (slot, member) words of
            // prologue and epilogue, theta, A and length rows gathered per (slot, member), the sums added per (slot,
            // member); per locus with a slot theta' and two totals stored and - several slots - a row zeroed; block sums.
            // No slot rows, no M-step vectors.
            const uint64_t tH = em->plan.tH;
            const uint64_t with_slot = tl.n_dest_rows ? std::min<uint64_t>(rows, em->L) : std::min<uint64_t>(tl.n_slots, em->L);
            info->estep_bytes = 4 * tl.n_batches * 64 + 16 * tl.n_tiles + 4 * tl.n_slots * 3 + 4 * rows * 2 +
                                8 * rows * tH * ((em->has_len ? 3 : 2) + 1) + 8 * with_slot * tH + 16 * with_slot +
                                8 * (tl.n_light) * tH + 16 * tl.n_tiles * TILE_WAVES +
                                (tl.n_sets ? 8 * tl.n_slots : 0);
            info->bytes_per_iter = info->estep_bytes;
        }
    }
    info->last_estep_ms = em->last_estep_ms;
    info->last_step_ms = em->last_step_ms;
    info->num_loci = em->L;
    info->num_haps = em->H;
    info->layout = em->layout;
    info->retained_build_bytes = em->tl.retired_bytes;
    info->num_locus_sets = em->layout == 1 ? em->tl.n_sets : 0;
    return GBRS_OK;
}

int gbrs_em_fold_counts(gbrs_em_t *em, uint64_t *one_word_reads, uint64_t *two_word_reads) {
    if (!em || !one_word_reads || !two_word_reads) return fail(GBRS_ERR_INVALID, "NULL argument");
    *one_word_reads = em->layout == 1 ? em->tl.n_folded : 0;
    *two_word_reads = em->layout == 1 ? em->tl.n_folded_two : 0;
    return GBRS_OK;
}

int gbrs_em_tile_cut(gbrs_em_t *em, uint32_t *passes, uint32_t *tile_words) {
    if (!em || !passes || !tile_words) return fail(GBRS_ERR_INVALID, "NULL argument");
    *passes = em->layout == 1 ? em->tl.cut_passes : 0;
    *tile_words = em->layout == 1 ? em->tl.cut_tile_words : 0;
    return GBRS_OK;
}

int gbrs_em_gather_mstep(gbrs_em_t *em, uint32_t *taken) {
    if (!em || !taken) return fail(GBRS_ERR_INVALID, "NULL argument");
    *taken = em_gather_route(em) ? 1u : 0u;
    return GBRS_OK;
}

int gbrs_em_tile_shapes(gbrs_em_t *em, uint32_t *n_batches, uint32_t *dict_entries, uint64_t n) {
    if (!em || !n_batches || !dict_entries) return fail(GBRS_ERR_INVALID, "NULL argument");
    if (em->layout != 1 || n != em->tl.n_tiles) return fail(GBRS_ERR_INVALID, "n is not the handle's number of tiles");
    (void)hipSetDevice(em->device);
    std::vector<TileHdr> hdr(n);
    if (n) GBRS_HIP_CHECK(hipMemcpy(hdr.data(), em->tl.tiles.p, n * sizeof(TileHdr), hipMemcpyDeviceToHost));
    for (uint64_t t = 0; t < n; ++t) {
        n_batches[t] = hdr[t].n_batches;
        dict_entries[t] = hdr[t].dict_count();
    }
    return GBRS_OK;
}

// A host walk over the counted batches of every tile, as the wavefronts' shares of em_tiles.inc see them: wavefront w of
// a tile takes batches [nb w / 8, nb (w + 1) / 8), and its lanes know no dictionary entry when it starts.
int gbrs_em_stripe_census(gbrs_em_t *em, uint32_t S, uint64_t *out) {
    if (!em || !out) return fail(GBRS_ERR_INVALID, "NULL argument");
    for (int k = 0; k < 6; ++k) out[k] = 0;
    if (em->layout != 1 || em->tl.n_tiles == 0) return GBRS_OK;
    (void)hipSetDevice(em->device);
    const TileLayout &tl = em->tl;
    std::vector<TileHdr> hdr(tl.n_tiles);
    std::vector<uint32_t> words((size_t)tl.n_batches * 64);
    GBRS_HIP_CHECK(hipMemcpy(hdr.data(), tl.tiles.p, hdr.size() * sizeof(TileHdr), hipMemcpyDeviceToHost));
    if (!words.empty()) GBRS_HIP_CHECK(hipMemcpy(words.data(), tl.words.p, words.size() * 4, hipMemcpyDeviceToHost));
    const uint32_t H = em->plan.tH, shift = H + 2 * pos_bits((int)H), hmask = (1u << H) - 1u;
    for (const TileHdr &th : hdr) {
        const uint32_t nb = th.n_batches, lead = std::min<uint32_t>(th.n_one + th.n_two(), nb);
        if ((uint64_t)th.batch_base + nb > tl.n_batches) return fail(GBRS_ERR_STATE, "a tile header is out of range");
        const uint32_t *w = words.data() + (size_t)th.batch_base * 64;
        for (uint32_t b = 0; b < lead; ++b)
            for (int l = 0; l < 64; ++l) out[4] += (w[(size_t)b * 64 + l] & hmask) == 0u;
        out[0] += lead;
        for (int wave = 0; wave < TILE_WAVES; ++wave) {
            const uint32_t b0 = (uint32_t)(((uint64_t)nb * wave) / TILE_WAVES), b1 = (uint32_t)(((uint64_t)nb * (wave + 1)) / TILE_WAVES);
            if (b0 < b1 && b0 < lead) ++out[1];
            for (uint32_t b = b0 + 1; b < std::min(b1, lead); ++b) {
                uint32_t lanes = 0;
                for (int l = 0; l < 64; ++l) lanes += (w[(size_t)b * 64 + l] >> shift) != (w[(size_t)(b - 1) * 64 + l] >> shift);
                if (!lanes) continue;
                ++out[2];
                out[3] += lanes;
                const uint32_t first = b < th.n_one ? 0u : th.n_one;
                if (S != 0 && (b - first) % S != 0) ++out[5];
            }
        }
    }
    return GBRS_OK;
}

int gbrs_counts_create(uint64_t R, uint32_t L, uint32_t H, const uint32_t *const *indptr,
                       const uint32_t *const *indices, const double *count, int device, gbrs_counts_t **out) {
    if (!out) return fail(GBRS_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (H < 1 || H > 32 || L < 1 || R < 1 || R > 0xFFFFFFFFull || !indptr || !indices)
        return fail(GBRS_ERR_INVALID, "The shape must be a tuple of three positive integers (H <= 32, R < 2^32).");
    GBRS_TRY(select_device(device));
    gbrs_counts *c = new gbrs_counts();
    struct Guard { gbrs_counts *p; ~Guard() { if (p) gbrs_counts_destroy(p); } } guard{c};
    c->device = device;
    c->R = R; c->L = L; c->H = H;
    GBRS_HIP_CHECK(hipStreamCreateWithFlags(&c->s, hipStreamDefault));
    GBRS_TRY(upload_csc(R, L, H, indptr, indices, false, c->ent_row, c->col_ptr, c->n));
    if (count) {
        GBRS_TRY(c->d_count.alloc(R));
        GBRS_HIP_CHECK(hipMemcpy(c->d_count.p, count, R * sizeof(double), hipMemcpyHostToDevice));
    }
    GBRS_HIP_CHECK(hipDeviceSynchronize());
    GBRS_TRY(check_row_ids(c->n, c->ent_row.p, R, c->s));
    c->work = counts_work_new();
    guard.p = nullptr;
    *out = c;
    return GBRS_OK;
}

int gbrs_counts_get(gbrs_counts_t *c, const int32_t *locus_group, uint32_t num_out_loci, double *aln_counts,
                    double *allele_unique, double *locus_unique) {
    RoctxRange roctx_range("gbrs_counts_get");
    if (!c) return fail(GBRS_ERR_INVALID, "handle is NULL");
    const uint32_t L = c->L, H = c->H;
    const uint32_t Lout = locus_group ? num_out_loci : L;
    if (Lout < 1 || Lout >= (1u << 27)) return fail(GBRS_ERR_INVALID, "bad number of output loci");
    if (locus_group)
        for (uint32_t l = 0; l < L; ++l)
            if (locus_group[l] < -1 || (locus_group[l] >= 0 && (uint32_t)locus_group[l] >= Lout))
                return fail(GBRS_ERR_INVALID, "locus_group[%u] out of range", l);
    GBRS_TRY(select_device(c->device));
    DevBuf<double> d_aln, d_uniq, d_lu;
    DevBuf<int32_t> d_group;
    if (locus_group) {
        GBRS_TRY(d_group.alloc(L));
        GBRS_HIP_CHECK(hipMemcpy(d_group.p, locus_group, L * sizeof(int32_t), hipMemcpyHostToDevice));
    }
    GBRS_TRY(d_aln.alloc((size_t)H * Lout));
    GBRS_TRY(d_uniq.alloc((size_t)H * Lout));
    GBRS_TRY(d_lu.alloc(Lout));
    GBRS_TRY(alignment_counts_device(c->R, L, H, c->n, c->ent_row.p, c->col_ptr.p, c->d_count.p,
                                     locus_group ? d_group.p : nullptr, Lout, d_aln.p, d_uniq.p, d_lu.p, c->s, c->work));
    if (aln_counts) GBRS_HIP_CHECK(hipMemcpy(aln_counts, d_aln.p, d_aln.bytes(), hipMemcpyDeviceToHost));
    if (allele_unique) GBRS_HIP_CHECK(hipMemcpy(allele_unique, d_uniq.p, d_uniq.bytes(), hipMemcpyDeviceToHost));
    if (locus_unique) GBRS_HIP_CHECK(hipMemcpy(locus_unique, d_lu.p, d_lu.bytes(), hipMemcpyDeviceToHost));
    return GBRS_OK;
}

int gbrs_counts_destroy(gbrs_counts_t *c) {
    if (!c) return GBRS_OK;
    (void)hipSetDevice(c->device);
    if (c->s) {
        (void)hipStreamSynchronize(c->s);
        (void)hipStreamDestroy(c->s);
    }
    if (c->work) counts_work_free(c->work);
    delete c;
    return GBRS_OK;
}

int gbrs_alignment_counts(uint64_t R, uint32_t L, uint32_t H, const uint32_t *const *indptr,
                          const uint32_t *const *indices, const double *count, const int32_t *locus_group,
                          uint32_t num_out_loci, int device, double *aln_counts, double *allele_unique,
                          double *locus_unique) {
    gbrs_counts_t *c = nullptr;
    GBRS_TRY(gbrs_counts_create(R, L, H, indptr, indices, count, device, &c));
    const int st = gbrs_counts_get(c, locus_group, num_out_loci, aln_counts, allele_unique, locus_unique);
    (void)gbrs_counts_destroy(c);
    return st;
}

// ---- bootstrap replicates (GBRS_EM_RESAMPLE; kernels in em_resample.inc) ------------------------------------------
int gbrs_em_resample(gbrs_em_t *em, uint64_t seed, uint32_t replicate) {
    RoctxRange roctx_range("gbrs_em_resample");
    if (!em) return fail(GBRS_ERR_INVALID, "handle is NULL");
    if (!em->resample) return fail(GBRS_ERR_STATE, "the handle was not created with GBRS_EM_RESAMPLE");
    GBRS_TRY(select_device(em->device));
    GBRS_TRY(em_flush_err(em));
    const uint64_t R = em->R;
    const unsigned rgrid = (unsigned)((R + 255) / 256);
    const uint32_t *base = em->has_base ? em->base_count.p : (const uint32_t *)nullptr;
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    if (replicate == GBRS_RESAMPLE_BASE) {
        hipLaunchKernelGGL(resample_draw_kernel<true>, dim3(rgrid), dim3(256), 0, em->stream, R, base, 0u, 0u, 0u, 0u, em->count.p);
    } else {
        hipLaunchKernelGGL(resample_draw_kernel<false>, dim3(rgrid), dim3(256), 0, em->stream, R, base, em->plan.resample_cut,
                           replicate, k0, k1, em->count.p);
        if (em->n_big)
            hipLaunchKernelGGL(resample_big_kernel, dim3(em->n_big), dim3(256), 0, em->stream, em->n_big, em->big_rows.p, base,
                               replicate, k0, k1, em->count.p);
    }
    // the weights onto every structure the handle steps on: the tiles' words and the long rows (the CSC, models 1-3 and
    // posterior kernels read `count` itself; prepare runs on the same structures)
    const TileLayout &tl = em->tl;
    if (em->layout == 1 && tl.word_row.n)
        hipLaunchKernelGGL(install_weights_kernel, dim3((unsigned)((tl.word_row.n + 255) / 256)), dim3(256), 0, em->stream,
                           (uint64_t)tl.word_row.n, tl.word_row.p, em->count.p, tl.word_weight.p);
    if (em->layout == 1 && tl.long_row.n)
        hipLaunchKernelGGL(install_weights_kernel, dim3((unsigned)((tl.long_row.n + 255) / 256)), dim3(256), 0, em->stream,
                           (uint64_t)tl.long_row.n, tl.long_row.p, em->count.p, tl.long_weight.p);
    GBRS_HIP_CHECK(hipGetLastError());
    em->prepared = false;                     // theta belongs to other weights: prepare comes next
    em->post_model = 0;
    GBRS_HIP_CHECK(hipStreamSynchronize(em->stream));
    return GBRS_OK;
}

int gbrs_em_weights(gbrs_em_t *em, double *out) {
    if (!em || !out) return fail(GBRS_ERR_INVALID, "NULL argument");
    if (!em->resample) return fail(GBRS_ERR_STATE, "the handle was not created with GBRS_EM_RESAMPLE");
    GBRS_TRY(select_device(em->device));
    GBRS_HIP_CHECK(hipMemcpyAsync(out, em->count.p, em->R * sizeof(double), hipMemcpyDeviceToHost, em->stream));
    GBRS_HIP_CHECK(hipStreamSynchronize(em->stream));
    return GBRS_OK;
}

int gbrs_em_resample_info(gbrs_em_t *em, uint64_t *extra_device_bytes, uint64_t *num_big_rows, uint32_t *cut) {
    if (!em) return fail(GBRS_ERR_INVALID, "handle is NULL");
    if (!em->resample) return fail(GBRS_ERR_STATE, "the handle was not created with GBRS_EM_RESAMPLE");
    if (extra_device_bytes)
        *extra_device_bytes = em->base_count.bytes() + em->big_rows.bytes() + em->tl.word_row.bytes() + em->tl.long_row.bytes() +
                              (em->has_base ? 0 : em->count.bytes() + em->tl.word_weight.bytes() + em->tl.long_weight.bytes());
    if (num_big_rows) *num_big_rows = em->n_big;
    if (cut) *cut = em->plan.resample_cut;
    return GBRS_OK;
}

int gbrs_em_bootstrap_begin(gbrs_em_t *em, int64_t G, const int64_t *group_ptr, const int64_t *members) {
    if (!em) return fail(GBRS_ERR_INVALID, "handle is NULL");
    if (G < 0 || (G > 0 && (!group_ptr || !members))) return fail(GBRS_ERR_INVALID, "bad group arguments");
    GBRS_TRY(select_device(em->device));
    gbrs_em::Stats &st = em->stats;
    st.active = false;
    st.n = 0;
    st.G = G;
    if (G > 0) {
        const int64_t nm = group_ptr[G];
        for (int64_t g = 0; g < G; ++g)
            if (group_ptr[g + 1] < group_ptr[g]) return fail(GBRS_ERR_INVALID, "group_ptr not monotone");
        for (int64_t k = 0; k < nm; ++k)
            if (members[k] < 0 || members[k] >= (int64_t)em->L)
                return fail(GBRS_ERR_INVALID, "group member %lld out of range", (long long)members[k]);
        GBRS_TRY(st.gptr.alloc(G + 1));
        GBRS_TRY(st.gmem.alloc(std::max<int64_t>(nm, 1)));
        GBRS_HIP_CHECK(hipMemcpy(st.gptr.p, group_ptr, (G + 1) * sizeof(int64_t), hipMemcpyHostToDevice));
        if (nm) GBRS_HIP_CHECK(hipMemcpy(st.gmem.p, members, nm * sizeof(int64_t), hipMemcpyHostToDevice));
    }
    GBRS_TRY(st.theta_sum.alloc(1));
    for (int level = 0; level < 2; ++level) {
        const size_t n = level == 0 ? em->L : (size_t)G;
        for (int q = 0; q < 2; ++q) {
            GBRS_TRY(st.cur[level][q].alloc(n * em->H));
            GBRS_TRY(st.mean[level][q].alloc(n * em->H));
            GBRS_TRY(st.m2[level][q].alloc(n * em->H));
            GBRS_TRY(st.tot_mean[level][q].alloc(n));
            GBRS_TRY(st.tot_m2[level][q].alloc(n));
        }
    }
    st.active = true;
    return GBRS_OK;
}

int gbrs_em_bootstrap_add(gbrs_em_t *em, double *tpm, double *counts, double *gene_tpm, double *gene_counts) {
    if (!em) return fail(GBRS_ERR_INVALID, "handle is NULL");
    gbrs_em::Stats &st = em->stats;
    if (!st.active) return fail(GBRS_ERR_STATE, "gbrs_em_bootstrap_begin has not been called");
    if (!em->prepared) return fail(GBRS_ERR_STATE, "prepare() has not been called");
    if ((gene_tpm || gene_counts) && st.G == 0) return fail(GBRS_ERR_INVALID, "gene-level values were asked for without groups");
    GBRS_TRY(select_device(em->device));
    GBRS_TRY(em_flush_err(em));
    GBRS_TRY(em_refresh_counts(em));
    const uint32_t L = em->L, H = em->H;
    const uint64_t HL = (uint64_t)L * H;
    hipStream_t s = em->stream;
    st.n += 1;
    hipLaunchKernelGGL(stats_sum_kernel, dim3(1), dim3(1024), 0, s, HL, em->theta.p, st.theta_sum.p);
    hipLaunchKernelGGL(stats_current_kernel, dim3((unsigned)((HL + 255) / 256)), dim3(256), 0, s, L, H, em->theta.p, em->counts.p,
                       st.theta_sum.p, st.cur[0][0].p, st.cur[0][1].p);
    for (int q = 0; q < 2; ++q) {
        hipLaunchKernelGGL(stats_fold_kernel, dim3((L + 255) / 256), dim3(256), 0, s, (uint64_t)L, H, st.n, st.cur[0][q].p,
                           st.mean[0][q].p, st.m2[0][q].p, st.tot_mean[0][q].p, st.tot_m2[0][q].p);
        if (st.G > 0) {
            const int64_t total = st.G * (int64_t)H;
            hipLaunchKernelGGL(stats_group_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, L, H, st.G, st.gptr.p,
                               st.gmem.p, st.cur[0][q].p, st.cur[1][q].p);
            hipLaunchKernelGGL(stats_fold_kernel, dim3((unsigned)((st.G + 255) / 256)), dim3(256), 0, s, (uint64_t)st.G, H, st.n,
                               st.cur[1][q].p, st.mean[1][q].p, st.m2[1][q].p, st.tot_mean[1][q].p, st.tot_m2[1][q].p);
        }
    }
    GBRS_HIP_CHECK(hipGetLastError());
    double *outs[2][2] = {{tpm, counts}, {gene_tpm, gene_counts}};
    for (int level = 0; level < 2; ++level)
        for (int q = 0; q < 2; ++q)
            if (outs[level][q] && st.cur[level][q].n)
                GBRS_HIP_CHECK(hipMemcpyAsync(outs[level][q], st.cur[level][q].p, st.cur[level][q].bytes(), hipMemcpyDeviceToHost, s));
    GBRS_HIP_CHECK(hipStreamSynchronize(s));
    return GBRS_OK;
}

int gbrs_em_bootstrap_get(gbrs_em_t *em, int level, uint32_t *num_replicates, double *tpm_mean, double *tpm_sd,
                          double *count_mean, double *count_sd, double *tpm_total_mean, double *tpm_total_sd,
                          double *count_total_mean, double *count_total_sd) {
    if (!em) return fail(GBRS_ERR_INVALID, "handle is NULL");
    gbrs_em::Stats &st = em->stats;
    if (!st.active) return fail(GBRS_ERR_STATE, "gbrs_em_bootstrap_begin has not been called");
    if (level != 0 && level != 1) return fail(GBRS_ERR_INVALID, "level is 0 (isoforms) or 1 (genes)");
    if (level == 1 && st.G == 0) return fail(GBRS_ERR_INVALID, "gene-level statistics were asked for without groups");
    if (num_replicates) *num_replicates = st.n;
    if (st.n == 0) return fail(GBRS_ERR_STATE, "no replicate has been added");
    GBRS_TRY(select_device(em->device));
    GBRS_HIP_CHECK(hipStreamSynchronize(em->stream));
    // the standard deviation with B - 1 in the denominator (one replicate: NaN, as numpy.std(ddof=1) gives)
    const double denom = (double)st.n - 1.0;
    auto fetch = [&](const DevBuf<double> &mean, const DevBuf<double> &m2, double *mean_out, double *sd_out) -> int {
        if (mean_out && mean.n) GBRS_HIP_CHECK(hipMemcpy(mean_out, mean.p, mean.bytes(), hipMemcpyDeviceToHost));
        if (sd_out && m2.n) {
            GBRS_HIP_CHECK(hipMemcpy(sd_out, m2.p, m2.bytes(), hipMemcpyDeviceToHost));
            for (size_t i = 0; i < m2.n; ++i) sd_out[i] = std::sqrt(sd_out[i] / denom);
        }
        return GBRS_OK;
    };
    GBRS_TRY(fetch(st.mean[level][0], st.m2[level][0], tpm_mean, tpm_sd));
    GBRS_TRY(fetch(st.mean[level][1], st.m2[level][1], count_mean, count_sd));
    GBRS_TRY(fetch(st.tot_mean[level][0], st.tot_m2[level][0], tpm_total_mean, tpm_total_sd));
    GBRS_TRY(fetch(st.tot_mean[level][1], st.tot_m2[level][1], count_total_mean, count_total_sd));
    return GBRS_OK;
}

int gbrs_em_destroy(gbrs_em_t *em) {
    if (!em) return GBRS_OK;
    (void)hipSetDevice(em->device);
    if (em->stream) (void)hipStreamSynchronize(em->stream);
    for (auto e : em->ev_pool) if (e) (void)hipEventDestroy(e);
    if (em->pair_ev_mstep) (void)hipEventDestroy(em->pair_ev_mstep);
    if (em->pair_ev_err) (void)hipEventDestroy(em->pair_ev_err);
    if (em->stream && em->own_stream) (void)hipStreamDestroy(em->stream);
    delete em;
    return GBRS_OK;
}

}  // extern "C"

// gbrs_warm_up (common.hip): loads this file's code object
namespace gbrs {
__global__ void warm_em_kernel() {}
void warm_em(hipStream_t st) { hipLaunchKernelGGL(warm_em_kernel, dim3(1), dim3(64), 0, st); }
}  // namespace gbrs
