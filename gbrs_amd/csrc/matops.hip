// Structure edits of one sample's alignment incidence tensor on the device (gbrs_matops_*, include/gbrs_hip.h): the
// numeric bodies of `get-common-alignments`, `combine`, `pull-out-unique-reads` and `stencil`.
//
// The handle keeps, per haplotype, the CSC arrays of the (R x L) incidence matrix: ip uint32[L + 1] and ix uint32[nnz]
// with the row ids ASCENDING inside every column.  That order is an invariant of the handle: every operand (the arrays
// given to create, intersect and append_rows) goes through one check pass that range-checks its row ids and tells
// whether its columns ascend already; an operand whose columns do not is put in order once, by a 64-bit radix sort of
// (column << 32 | row) keys (the "general route"), and from there on every operation is the sorted one:
//   intersect        one thread per entry of m: its column by a binary search in ip, then a binary search for its row
//                    id in the same column of b; flag -> scan -> compact
//   append_rows      one thread per entry of either operand, written straight to its place: column of m first, then
//                    the column of b with the row offset added, which keeps the columns ascending
//   keep_unique_rows two 32-bit atomics (min, max of the entry's locus / gene / (haplotype, gene) key) per entry into
//                    uint32[R] arrays, a row is unique when it was seen and min == max; flag -> scan -> compact
//   mask_columns     flag by (haplotype, column) bit; flag -> scan -> compact
// The new column pointers are the exclusive scan of the flags read at the old column pointers, so a column of any
// length is as parallel as the rest and survivors keep their order.  Every row id is compared with R before anything
// is indexed with it and every column pointer table is checked on the host before a kernel reads at it.
//
// shared_counts (`count-shared-multireads-pairwise`) reads the tensor and leaves it as it is.  With P the R x n pattern
// matrix (P[r, c] = 1 when read r has an entry at column c - a locus, or a group of loci - in any haplotype) it
// computes C = P^T P, held as sorted (i, j) keys with integer counts:
//   1. one key (row << cb | column) per stored entry of every haplotype, cb = the bits of a column id, the column
//      mapped through locus_group and an entry of a locus in no group given the key of row R; radix sort, unique: P in
//      row order, the leftover key of row R cut off
//   2. entry k of P pairs with itself and with the entries after it in its row: cnt[k] = row end - k (galloping search
//      for the row end), exclusive scan in uint64: off[k], off[N] = the number of pairs (i <= j) of the whole sample
//   3. the pair index space [0, off[N]) is cut into batches of at most `budget` pairs.  One thread per pair: entry k by a
//      binary search in off, partner k + (p - off[k]).  A batch boundary may fall anywhere, inside a row as well, so a
//      read with hundreds of loci is as parallel as the rest and a row whose pairs exceed the budget needs nothing special
//   4. per batch: radix sort of the (i << cb | j) keys, reduce_by_key with a constant 1 -> distinct keys with uint32
//      counts; the reduced batch is merged into the running result by sort_pairs + reduce_by_key (the segmented sum)
//   5. mirror the strict upper triangle, sort_pairs, row pointers by binary search: CSR, column ids ascending
// Counts are uint32 throughout (a count is at most R < 2^32) and become doubles in the copy out; nothing is added with
// atomics, so a result does not depend on the run.
#include "prim.h"

#include <algorithm>

namespace gbrs {
namespace {

constexpr unsigned MO_BLOCK = 256;
constexpr uint32_t MO_MAX_HAPS = 32;

inline unsigned mo_grid(uint64_t n) {
    const uint64_t g = (n + MO_BLOCK - 1) / MO_BLOCK;
    return (unsigned)std::min<uint64_t>(std::max<uint64_t>(g, 1), 65536);
}

// the column l with ip[l] <= k < ip[l + 1]; needs ip[0] == 0 <= k < ip[L] (checked by the callers: k < nnz == ip[L])
__device__ __forceinline__ uint32_t mo_column_of(const uint32_t *__restrict__ ip, uint32_t L, uint32_t k) {
    uint32_t lo = 0, hi = L;
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (ip[mid] <= k) lo = mid;
        else hi = mid;
    }
    return lo;
}

// state bit 1: some column does not ascend strictly; bit 2: a row id >= R
__global__ void __launch_bounds__(MO_BLOCK)
mo_check_kernel(uint64_t n, const uint32_t *__restrict__ ix, uint64_t R, const uint32_t *__restrict__ ip, uint32_t L,
                uint32_t *__restrict__ state) {
    uint32_t local = 0;
    for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t r = ix[k];
        if (r >= R) local |= 2u;
        if (k > 0 && r <= ix[k - 1] && !(local & 1u)) {
            // a step down is in order only where a column starts
            const uint32_t l = mo_column_of(ip, L, (uint32_t)k);
            if (ip[l] != (uint32_t)k) local |= 1u;
        }
    }
    const uint32_t any = (__ballot(local & 1u) ? 1u : 0u) | (__ballot(local & 2u) ? 2u : 0u);
    if ((threadIdx.x & 63) == 0 && any) atomicOr(state, any);
}

__global__ void __launch_bounds__(MO_BLOCK)
mo_make_keys_kernel(uint64_t n, const uint32_t *__restrict__ ix, const uint32_t *__restrict__ ip, uint32_t L,
                    uint64_t *__restrict__ keys) {
    for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (uint64_t)gridDim.x * blockDim.x)
        keys[k] = ((uint64_t)mo_column_of(ip, L, (uint32_t)k) << 32) | ix[k];
}

__global__ void __launch_bounds__(MO_BLOCK)
mo_unpack_keys_kernel(uint64_t n, const uint64_t *__restrict__ keys, uint32_t *__restrict__ ix) {
    for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (uint64_t)gridDim.x * blockDim.x)
        ix[k] = (uint32_t)keys[k];
}

// flag[k] = entry k of a is also in b (same column, same row); flag[n] = 0 closes the exclusive scan
__global__ void __launch_bounds__(MO_BLOCK)
mo_intersect_flag_kernel(uint64_t n, const uint32_t *__restrict__ ixa, const uint32_t *__restrict__ ipa, uint32_t L,
                         const uint32_t *__restrict__ ixb, const uint32_t *__restrict__ ipb,
                         uint32_t *__restrict__ flag) {
    for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k <= n; k += (uint64_t)gridDim.x * blockDim.x) {
        uint32_t f = 0;
        if (k < n) {
            const uint32_t r = ixa[k];
            const uint32_t l = mo_column_of(ipa, L, (uint32_t)k);
            uint32_t lo = ipb[l], hi = ipb[l + 1];          // first j in [lo, hi) with ixb[j] >= r
            const uint32_t end = hi;
            while (lo < hi) {
                const uint32_t mid = lo + (hi - lo) / 2;
                if (ixb[mid] < r) lo = mid + 1;
                else hi = mid;
            }
            f = (lo < end && ixb[lo] == r) ? 1u : 0u;
        }
        flag[k] = f;
    }
}

// key of an entry: locus (or gene) id, or haplotype * G + that; entries of loci in no group are skipped.
// ix was range-checked against R when the operand was uploaded.
__global__ void __launch_bounds__(MO_BLOCK)
mo_row_key_kernel(uint64_t n, const uint32_t *__restrict__ ix, const uint32_t *__restrict__ ip, uint32_t L,
                  const int32_t *__restrict__ locus_group, uint32_t key_base, uint32_t *__restrict__ rmin,
                  uint32_t *__restrict__ rmax) {
    for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t l = mo_column_of(ip, L, (uint32_t)k);
        int32_t g = (int32_t)l;
        if (locus_group) {
            g = locus_group[l];
            if (g < 0) continue;
        }
        const uint32_t key = key_base + (uint32_t)g;
        const uint32_t r = ix[k];
        atomicMin(&rmin[r], key);
        atomicMax(&rmax[r], key);
    }
}

// rmin starts at 0xFFFFFFFF and rmax at 0, every key is below 0xFFFFFFFF: an unseen row has min > max
__global__ void __launch_bounds__(MO_BLOCK)
mo_keep_rows_kernel(uint64_t R, const uint32_t *__restrict__ rmin, const uint32_t *__restrict__ rmax,
                    uint8_t *__restrict__ keep) {
    for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r < R; r += (uint64_t)gridDim.x * blockDim.x)
        keep[r] = rmin[r] == rmax[r] ? 1 : 0;
}

__global__ void __launch_bounds__(MO_BLOCK)
mo_row_flag_kernel(uint64_t n, const uint32_t *__restrict__ ix, const uint8_t *__restrict__ keep,
                   uint32_t *__restrict__ flag) {
    for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k <= n; k += (uint64_t)gridDim.x * blockDim.x)
        flag[k] = k < n ? (uint32_t)keep[ix[k]] : 0u;
}

__global__ void __launch_bounds__(MO_BLOCK)
mo_column_flag_kernel(uint64_t n, const uint32_t *__restrict__ ip, uint32_t L, const uint32_t *__restrict__ allowed,
                      uint32_t h, uint32_t *__restrict__ flag) {
    for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k <= n; k += (uint64_t)gridDim.x * blockDim.x)
        flag[k] = k < n ? ((allowed[mo_column_of(ip, L, (uint32_t)k)] >> h) & 1u) : 0u;
}

__global__ void __launch_bounds__(MO_BLOCK)
mo_compact_kernel(uint64_t n, const uint32_t *__restrict__ ix, const uint32_t *__restrict__ flag,
                  const uint32_t *__restrict__ pos, uint32_t *__restrict__ out) {
    for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (uint64_t)gridDim.x * blockDim.x)
        if (flag[k]) out[pos[k]] = ix[k];
}

__global__ void __launch_bounds__(MO_BLOCK)
mo_indptr_kernel(uint32_t L, const uint32_t *__restrict__ ip, const uint32_t *__restrict__ pos,
                 uint32_t *__restrict__ ip_out) {
    for (uint64_t l = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; l <= L; l += (uint64_t)gridDim.x * blockDim.x)
        ip_out[l] = pos[ip[l]];
}

// entry k of column l of `src` goes to out[k + shift[l + first]] with `add` added to its row id: for the entries of m
// shift = ip of b, first = 0 (the entries of b's earlier columns come before it); for the entries of b shift = ip of
// m, first = 1 (all of m's columns up to and including l come before it)
__global__ void __launch_bounds__(MO_BLOCK)
mo_append_kernel(uint64_t n, const uint32_t *__restrict__ ix, const uint32_t *__restrict__ ip, uint32_t L,
                 const uint32_t *__restrict__ shift, uint32_t first, uint32_t add, uint32_t *__restrict__ out) {
    for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t l = mo_column_of(ip, L, (uint32_t)k);
        out[k + shift[l + first]] = ix[k] + add;
    }
}

__global__ void __launch_bounds__(MO_BLOCK)
mo_add_indptr_kernel(uint32_t L, const uint32_t *__restrict__ a, const uint32_t *__restrict__ b,
                     uint32_t *__restrict__ out) {
    for (uint64_t l = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; l <= L; l += (uint64_t)gridDim.x * blockDim.x)
        out[l] = a[l] + b[l];
}

// ---- shared_counts ---------------------------------------------------------------------------------------------
// (row << cb | column) of every entry of one haplotype, the column mapped through locus_group; an entry of a locus in
// no group gets row R, which sorts behind every real row.  ix was range-checked against R at the upload.
__global__ void __launch_bounds__(MO_BLOCK)
sc_entry_keys_kernel(uint64_t n, const uint32_t *__restrict__ ix, const uint32_t *__restrict__ ip, uint32_t L,
                     const int32_t *__restrict__ locus_group, uint64_t R, uint32_t cb, uint64_t *__restrict__ keys) {
    for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t l = mo_column_of(ip, L, (uint32_t)k);
        int64_t g = l;
        if (locus_group) g = locus_group[l];
        keys[k] = g < 0 ? (R << cb) : (((uint64_t)ix[k] << cb) | (uint64_t)g);
    }
}

// cnt[k] = entries of k's row from k on = the pairs (i <= j) whose first column is entry k's; cnt[n] = 0 closes the
// scan.  The row end is found by doubling steps and a binary search inside the last step: O(log row length).
__global__ void __launch_bounds__(MO_BLOCK)
sc_pair_count_kernel(uint64_t n, const uint64_t *__restrict__ keys, uint32_t cb, uint64_t *__restrict__ cnt) {
    for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k <= n; k += (uint64_t)gridDim.x * blockDim.x) {
        if (k == n) {
            cnt[k] = 0;
            continue;
        }
        const uint64_t row = keys[k] >> cb;
        uint64_t lo = k, hi, step = 1;                  // lo is in the row; hi == n or is not
        for (;;) {
            hi = lo + step;
            if (hi >= n) { hi = n; break; }
            if ((keys[hi] >> cb) != row) break;
            lo = hi;
            step <<= 1;
        }
        while (hi - lo > 1) {
            const uint64_t mid = lo + (hi - lo) / 2;
            if ((keys[mid] >> cb) == row) lo = mid;
            else hi = mid;
        }
        cnt[k] = hi - k;
    }
}

// pair p of the sample, p in [p0, p0 + count): the entry k with off[k] <= p < off[k + 1] and the entry p - off[k]
// places after it, which cnt made sure is in the same row and below n.  off[0] = 0 and off[n] > p.
__global__ void __launch_bounds__(MO_BLOCK)
sc_emit_kernel(uint64_t p0, uint64_t count, const uint64_t *__restrict__ off, uint64_t n,
               const uint64_t *__restrict__ keys, uint32_t cb, uint64_t *__restrict__ out) {
    const uint64_t mask = (1ull << cb) - 1;
    for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < count; t += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t p = p0 + t;
        uint64_t lo = 0, hi = n;
        while (hi - lo > 1) {
            const uint64_t mid = lo + (hi - lo) / 2;
            if (off[mid] <= p) lo = mid;
            else hi = mid;
        }
        const uint64_t i = keys[lo] & mask, j = keys[lo + (p - off[lo])] & mask;
        out[t] = (i << cb) | j;
    }
}

// (i, j) with i <= j -> itself and (j, i); the second copy of a diagonal entry gets row n_cols, which sorts last
__global__ void __launch_bounds__(MO_BLOCK)
sc_mirror_kernel(uint64_t n, const uint64_t *__restrict__ keys, const uint32_t *__restrict__ cnt, uint32_t cb,
                 uint64_t n_cols, uint64_t *__restrict__ okeys, uint32_t *__restrict__ ocnt) {
    const uint64_t mask = (1ull << cb) - 1;
    for (uint64_t u = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; u < n; u += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t key = keys[u], i = key >> cb, j = key & mask;
        okeys[2 * u] = key;
        okeys[2 * u + 1] = i == j ? (n_cols << cb) : ((j << cb) | i);
        ocnt[2 * u] = ocnt[2 * u + 1] = cnt[u];
    }
}

// indptr[i] = the first of the n sorted keys whose row is >= i, for i in [0, n_cols]
__global__ void __launch_bounds__(MO_BLOCK)
sc_indptr_kernel(uint64_t n_cols, const uint64_t *__restrict__ keys, uint64_t n, uint32_t cb,
                 uint64_t *__restrict__ indptr) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i <= n_cols; i += (uint64_t)gridDim.x * blockDim.x) {
        uint64_t lo = 0, hi = n;
        while (lo < hi) {
            const uint64_t mid = lo + (hi - lo) / 2;
            if ((keys[mid] >> cb) < i) lo = mid + 1;
            else hi = mid;
        }
        indptr[i] = lo;
    }
}

__global__ void __launch_bounds__(MO_BLOCK)
sc_unpack_kernel(uint64_t n, const uint64_t *__restrict__ keys, const uint32_t *__restrict__ cnt, uint32_t cb,
                 uint32_t *__restrict__ indices, double *__restrict__ data) {
    const uint64_t mask = (1ull << cb) - 1;
    for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (uint64_t)gridDim.x * blockDim.x) {
        indices[k] = (uint32_t)(keys[k] & mask);
        data[k] = (double)cnt[k];
    }
}

#define MO_LAUNCH(kernel, n, s, ...)                                                                    \
    do {                                                                                                \
        hipLaunchKernelGGL(kernel, dim3(mo_grid(n)), dim3(MO_BLOCK), 0, s, __VA_ARGS__);                \
        GBRS_HIP_CHECK(hipGetLastError());                                                              \
    } while (0)

// one operand on the device: per haplotype ip[L + 1] and ix[nnz], columns ascending
struct MoOperand {
    DevBuf<uint32_t> ip[MO_MAX_HAPS], ix[MO_MAX_HAPS];
    uint64_t nnz[MO_MAX_HAPS] = {};
};

}  // namespace
}  // namespace gbrs

struct gbrs_matops {
    int device = 0;
    uint64_t R = 0;
    uint32_t L = 0, H = 0;
    hipStream_t stream = nullptr;
    gbrs::MoOperand m;
    gbrs::DevBuf<uint32_t> flag, pos, state;
    gbrs::Scratch sc;
    uint32_t sorted_inputs = 0;      // haplotype arrays of operands that took the general route so far
    // the last shared_counts result: keys (i << sc_cb | j) ascending = CSR order, their counts, the row pointers
    gbrs::DevBuf<uint64_t> sc_keys, sc_indptr;
    gbrs::DevBuf<uint32_t> sc_cnt;
    uint64_t sc_n = 0, sc_nnz = 0, sc_pattern = 0, sc_pairs = 0, sc_budget = 0, sc_peak = 0;
    uint32_t sc_cb = 0, sc_batches = 0;
    double sc_ms = 0.0;
    bool sc_valid = false;
};

namespace gbrs {
namespace {

int mo_shape_args(uint64_t R, uint32_t L, uint32_t H, const uint32_t *const *indptr, const uint32_t *const *indices) {
    if (R > 0xFFFFFFFFull) return fail(GBRS_ERR_UNSUPPORTED, "2^32 or more rows are not supported (%llu).", (unsigned long long)R);
    if (H < 1 || H > MO_MAX_HAPS || L < 1 || R < 1)
        return fail(GBRS_ERR_INVALID, "The shape must be a tuple of three positive integers (H <= 32, R < 2^32).");
    if (!indptr || !indices) return fail(GBRS_ERR_INVALID, "indptr/indices tables are NULL");
    for (uint32_t h = 0; h < H; ++h) {
        const uint32_t *p = indptr[h];
        if (!p) return fail(GBRS_ERR_INVALID, "indptr[%u] is NULL", h);
        if (p[0] != 0) return fail(GBRS_ERR_INVALID, "indptr[%u][0] != 0", h);
        for (uint32_t l = 0; l < L; ++l)
            if (p[l + 1] < p[l]) return fail(GBRS_ERR_INVALID, "indptr[%u] is not non-decreasing at %u", h, l);
        if (p[L] && !indices[h]) return fail(GBRS_ERR_INVALID, "indices[%u] is NULL", h);
    }
    return GBRS_OK;
}

// host arrays (validated by mo_shape_args) -> o, row ids checked against R, columns put in ascending order
int mo_upload(gbrs_matops *m, uint64_t R, const uint32_t *const *indptr, const uint32_t *const *indices, MoOperand &o) {
    const uint32_t L = m->L, H = m->H;
    hipStream_t s = m->stream;
    for (uint32_t h = 0; h < H; ++h) {
        const uint64_t n = indptr[h][L];
        o.nnz[h] = n;
        GBRS_TRY(o.ip[h].alloc((size_t)L + 1));
        GBRS_TRY(o.ix[h].alloc(std::max<uint64_t>(n, 1)));
        GBRS_HIP_CHECK(hipMemcpyAsync(o.ip[h].p, indptr[h], ((size_t)L + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, s));
        if (n) GBRS_HIP_CHECK(hipMemcpyAsync(o.ix[h].p, indices[h], n * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    }
    GBRS_HIP_CHECK(hipStreamSynchronize(s));      // the caller's arrays are not read after this point
    for (uint32_t h = 0; h < H; ++h) {
        const uint64_t n = o.nnz[h];
        if (!n) continue;
        GBRS_HIP_CHECK(hipMemsetAsync(m->state.p, 0, sizeof(uint32_t), s));
        MO_LAUNCH(mo_check_kernel, n, s, n, o.ix[h].p, R, o.ip[h].p, L, m->state.p);
        uint32_t st = 0;
        GBRS_HIP_CHECK(hipMemcpyAsync(&st, m->state.p, sizeof(st), hipMemcpyDeviceToHost, s));
        GBRS_HIP_CHECK(hipStreamSynchronize(s));
        if (st & 2u) return fail(GBRS_ERR_INVALID, "indices[%u] hold a row id >= num_rows", h);
        if (st & 1u) {      // general route: (column, row) keys through the radix sort
            DevBuf<uint64_t> keys, sorted;
            GBRS_TRY(keys.alloc(n));
            GBRS_TRY(sorted.alloc(n));
            MO_LAUNCH(mo_make_keys_kernel, n, s, n, o.ix[h].p, o.ip[h].p, L, keys.p);
            GBRS_TRY(sort_keys64(m->sc, keys.p, sorted.p, n, 32u + bits_for(L - 1), s));
            MO_LAUNCH(mo_unpack_keys_kernel, n, s, n, sorted.p, o.ix[h].p);
            GBRS_HIP_CHECK(hipStreamSynchronize(s));
            ++m->sorted_inputs;
        }
    }
    return GBRS_OK;
}

// m's haplotype h keeps the entries with flag 1 (m->flag holds nnz + 1 flags, the last one 0)
int mo_apply_flags(gbrs_matops *m, uint32_t h) {
    hipStream_t s = m->stream;
    const uint64_t n = m->m.nnz[h];
    GBRS_TRY(exclusive_scan(m->sc, m->flag.p, m->pos.p, n + 1, s));
    uint32_t kept = 0;
    GBRS_HIP_CHECK(hipMemcpyAsync(&kept, m->pos.p + n, sizeof(kept), hipMemcpyDeviceToHost, s));
    GBRS_HIP_CHECK(hipStreamSynchronize(s));
    DevBuf<uint32_t> ix, ip;
    GBRS_TRY(ix.alloc(std::max<uint64_t>(kept, 1)));
    GBRS_TRY(ip.alloc((size_t)m->L + 1));
    if (n) MO_LAUNCH(mo_compact_kernel, n, s, n, m->m.ix[h].p, m->flag.p, m->pos.p, ix.p);
    MO_LAUNCH(mo_indptr_kernel, (uint64_t)m->L + 1, s, m->L, m->m.ip[h].p, m->pos.p, ip.p);
    GBRS_HIP_CHECK(hipStreamSynchronize(s));
    m->m.ix[h].swap(ix);
    m->m.ip[h].swap(ip);
    m->m.nnz[h] = kept;
    return GBRS_OK;
}

int mo_reserve_flags(gbrs_matops *m) {
    uint64_t nmax = 0;
    for (uint32_t h = 0; h < m->H; ++h) nmax = std::max(nmax, m->m.nnz[h]);
    if (m->flag.n < nmax + 1) {
        GBRS_TRY(m->flag.alloc(nmax + 1));
        GBRS_TRY(m->pos.alloc(nmax + 1));
    }
    return GBRS_OK;
}

// the device bytes in use beyond `free0`, sampled after the large allocations of shared_counts
struct ScPeak {
    size_t free0 = 0;
    uint64_t peak = 0;
    void start() {
        size_t total = 0;
        if (hipMemGetInfo(&free0, &total) != hipSuccess) free0 = 0;
    }
    void sample() {
        size_t f = 0, total = 0;
        if (hipMemGetInfo(&f, &total) == hipSuccess && f < free0) peak = std::max<uint64_t>(peak, free0 - f);
    }
};

struct ScEvents {
    hipEvent_t a = nullptr, b = nullptr;
    ~ScEvents() {
        if (a) (void)hipEventDestroy(a);
        if (b) (void)hipEventDestroy(b);
    }
};

int sc_fetch(const uint64_t *d, uint64_t &v, hipStream_t s) {
    GBRS_HIP_CHECK(hipMemcpyAsync(&v, d, sizeof(v), hipMemcpyDeviceToHost, s));
    GBRS_HIP_CHECK(hipStreamSynchronize(s));
    return GBRS_OK;
}

// P in row order: the distinct (row << cb | column) keys of all haplotypes -> pk[0, N)
int sc_pattern(gbrs_matops *m, Scratch &sc, ScPeak &pm, const int32_t *d_group, uint32_t cb, DevBuf<uint64_t> &pk,
               uint64_t &N) {
    hipStream_t s = m->stream;
    uint64_t E = 0;
    for (uint32_t h = 0; h < m->H; ++h) E += m->m.nnz[h];
    N = 0;
    if (!E) return GBRS_OK;
    DevBuf<uint64_t> ek, es, d_count;
    GBRS_TRY(ek.alloc(E));
    GBRS_TRY(es.alloc(E));
    GBRS_TRY(d_count.alloc(1));
    uint64_t base = 0;
    for (uint32_t h = 0; h < m->H; ++h) {
        const uint64_t n = m->m.nnz[h];
        if (!n) continue;
        MO_LAUNCH(sc_entry_keys_kernel, n, s, n, m->m.ix[h].p, m->m.ip[h].p, m->L, d_group, m->R, cb, ek.p + base);
        base += n;
    }
    GBRS_TRY(sort_keys64(sc, ek.p, es.p, E, cb + bits_for(m->R), s));
    GBRS_TRY(unique_keys64(sc, es.p, ek.p, d_count.p, E, s));
    pm.sample();
    GBRS_TRY(sc_fetch(d_count.p, N, s));
    uint64_t last = 0;
    GBRS_TRY(sc_fetch(ek.p + (N - 1), last, s));
    if ((last >> cb) == m->R) --N;                      // the one key left of the entries in no group
    if (!N) return GBRS_OK;
    GBRS_TRY(pk.alloc(N));                              // a copy of the right size: the two E-sized arrays go back
    GBRS_HIP_CHECK(hipMemcpyAsync(pk.p, ek.p, N * sizeof(uint64_t), hipMemcpyDeviceToDevice, s));
    GBRS_HIP_CHECK(hipStreamSynchronize(s));
    return GBRS_OK;
}

// pairs per batch: GBRS_SHARED_PAIR_BUDGET, else 1/64 of the free device memory in pairs.  A pair costs 28 bytes while
// its batch is reduced (key, sorted key, the sort's own copy, count), which leaves the larger part to the merges.
int sc_budget(uint64_t &budget) {
    if (const char *e = std::getenv("GBRS_SHARED_PAIR_BUDGET")) {
        char *end = nullptr;
        const unsigned long long v = std::strtoull(e, &end, 10);
        if (!*e || *end || v < 1) return fail(GBRS_ERR_INVALID, "GBRS_SHARED_PAIR_BUDGET must be a positive number of pairs");
        budget = v;
        return GBRS_OK;
    }
    size_t f = 0, total = 0;
    GBRS_HIP_CHECK(hipMemGetInfo(&f, &total));
    budget = std::min<uint64_t>(std::max<uint64_t>(f / 64, 1ull << 20), 1ull << 31);
    return GBRS_OK;
}

}  // namespace
}  // namespace gbrs

extern "C" {

using namespace gbrs;

int gbrs_matops_create(uint64_t num_rows, uint32_t num_loci, uint32_t num_haps, const uint32_t *const *indptr,
                       const uint32_t *const *indices, int device, gbrs_matops_t **out) {
    RoctxRange roctx_range("gbrs_matops_create");
    if (!out) return fail(GBRS_ERR_INVALID, "out is NULL");
    *out = nullptr;
    GBRS_TRY(mo_shape_args(num_rows, num_loci, num_haps, indptr, indices));
    GBRS_TRY(select_device(device));
    gbrs_matops *m = new gbrs_matops();
    struct Guard { gbrs_matops *p; ~Guard() { if (p) gbrs_matops_destroy(p); } } guard{m};
    m->device = device; m->R = num_rows; m->L = num_loci; m->H = num_haps;
    GBRS_HIP_CHECK(hipStreamCreateWithFlags(&m->stream, hipStreamDefault));
    GBRS_TRY(m->state.alloc(1));
    GBRS_TRY(mo_upload(m, num_rows, indptr, indices, m->m));
    guard.p = nullptr;
    *out = m;
    return GBRS_OK;
}

int gbrs_matops_intersect(gbrs_matops_t *m, const uint32_t *const *indptr, const uint32_t *const *indices) {
    RoctxRange roctx_range("gbrs_matops_intersect");
    if (!m) return fail(GBRS_ERR_INVALID, "NULL handle");
    GBRS_TRY(mo_shape_args(m->R, m->L, m->H, indptr, indices));
    GBRS_TRY(select_device(m->device));
    MoOperand b;
    GBRS_TRY(mo_upload(m, m->R, indptr, indices, b));
    GBRS_TRY(mo_reserve_flags(m));
    for (uint32_t h = 0; h < m->H; ++h) {
        const uint64_t n = m->m.nnz[h];
        MO_LAUNCH(mo_intersect_flag_kernel, n + 1, m->stream, n, m->m.ix[h].p, m->m.ip[h].p, m->L, b.ix[h].p, b.ip[h].p,
                  m->flag.p);
        GBRS_TRY(mo_apply_flags(m, h));
    }
    return GBRS_OK;
}

int gbrs_matops_append_rows(gbrs_matops_t *m, uint64_t num_rows_b, const uint32_t *const *indptr,
                            const uint32_t *const *indices) {
    RoctxRange roctx_range("gbrs_matops_append_rows");
    if (!m) return fail(GBRS_ERR_INVALID, "NULL handle");
    GBRS_TRY(mo_shape_args(num_rows_b, m->L, m->H, indptr, indices));
    if (m->R + num_rows_b > 0xFFFFFFFFull)
        return fail(GBRS_ERR_UNSUPPORTED, "2^32 or more rows after the append are not supported.");
    for (uint32_t h = 0; h < m->H; ++h)
        if (m->m.nnz[h] + (uint64_t)indptr[h][m->L] > 0xFFFFFFFFull)
            return fail(GBRS_ERR_UNSUPPORTED, "2^32 or more entries of haplotype %u after the append are not supported.", h);
    GBRS_TRY(select_device(m->device));
    MoOperand b;
    GBRS_TRY(mo_upload(m, num_rows_b, indptr, indices, b));
    hipStream_t s = m->stream;
    const uint32_t L = m->L;
    for (uint32_t h = 0; h < m->H; ++h) {
        const uint64_t na = m->m.nnz[h], nb = b.nnz[h];
        DevBuf<uint32_t> ix, ip;
        GBRS_TRY(ix.alloc(std::max<uint64_t>(na + nb, 1)));
        GBRS_TRY(ip.alloc((size_t)L + 1));
        if (na) MO_LAUNCH(mo_append_kernel, na, s, na, m->m.ix[h].p, m->m.ip[h].p, L, b.ip[h].p, 0u, 0u, ix.p);
        if (nb) MO_LAUNCH(mo_append_kernel, nb, s, nb, b.ix[h].p, b.ip[h].p, L, m->m.ip[h].p, 1u, (uint32_t)m->R, ix.p);
        MO_LAUNCH(mo_add_indptr_kernel, (uint64_t)L + 1, s, L, m->m.ip[h].p, b.ip[h].p, ip.p);
        GBRS_HIP_CHECK(hipStreamSynchronize(s));
        m->m.ix[h].swap(ix);
        m->m.ip[h].swap(ip);
        m->m.nnz[h] = na + nb;
    }
    m->R += num_rows_b;
    return GBRS_OK;
}

int gbrs_matops_keep_unique_rows(gbrs_matops_t *m, const int32_t *locus_group, uint32_t num_groups,
                                 int ignore_haplotype, uint8_t *keep_out) {
    RoctxRange roctx_range("gbrs_matops_keep_unique_rows");
    if (!m) return fail(GBRS_ERR_INVALID, "NULL handle");
    const uint32_t L = m->L, H = m->H;
    const uint32_t G = locus_group ? num_groups : L;
    if (locus_group) {
        if (G < 1) return fail(GBRS_ERR_INVALID, "locus_group given with num_groups = 0");
        for (uint32_t l = 0; l < L; ++l)
            if (locus_group[l] < -1 || locus_group[l] >= (int64_t)G)
                return fail(GBRS_ERR_INVALID, "locus_group[%u] = %d is outside [-1, %u)", l, locus_group[l], G);
    }
    if ((uint64_t)H * G >= 0xFFFFFFFFull) return fail(GBRS_ERR_UNSUPPORTED, "(haplotype, group) keys do not fit 32 bits");
    GBRS_TRY(select_device(m->device));
    hipStream_t s = m->stream;
    DevBuf<uint32_t> rmin, rmax;
    DevBuf<int32_t> group;
    DevBuf<uint8_t> keep;
    GBRS_TRY(rmin.alloc(m->R));
    GBRS_TRY(rmax.alloc(m->R));
    GBRS_TRY(keep.alloc(m->R));
    GBRS_HIP_CHECK(hipMemsetAsync(rmin.p, 0xFF, rmin.bytes(), s));
    GBRS_HIP_CHECK(hipMemsetAsync(rmax.p, 0, rmax.bytes(), s));
    if (locus_group) {
        GBRS_TRY(group.alloc(L));
        GBRS_HIP_CHECK(hipMemcpyAsync(group.p, locus_group, (size_t)L * sizeof(int32_t), hipMemcpyHostToDevice, s));
    }
    for (uint32_t h = 0; h < H; ++h) {
        const uint64_t n = m->m.nnz[h];
        if (!n) continue;
        MO_LAUNCH(mo_row_key_kernel, n, s, n, m->m.ix[h].p, m->m.ip[h].p, L, locus_group ? group.p : (const int32_t *)nullptr,
                  ignore_haplotype ? 0u : h * G, rmin.p, rmax.p);
    }
    MO_LAUNCH(mo_keep_rows_kernel, m->R, s, m->R, rmin.p, rmax.p, keep.p);
    GBRS_TRY(mo_reserve_flags(m));
    for (uint32_t h = 0; h < H; ++h) {
        const uint64_t n = m->m.nnz[h];
        MO_LAUNCH(mo_row_flag_kernel, n + 1, s, n, m->m.ix[h].p, keep.p, m->flag.p);
        GBRS_TRY(mo_apply_flags(m, h));
    }
    if (keep_out) GBRS_HIP_CHECK(hipMemcpyAsync(keep_out, keep.p, m->R, hipMemcpyDeviceToHost, s));
    GBRS_HIP_CHECK(hipStreamSynchronize(s));
    return GBRS_OK;
}

int gbrs_matops_mask_columns(gbrs_matops_t *m, const uint32_t *allowed) {
    RoctxRange roctx_range("gbrs_matops_mask_columns");
    if (!m || !allowed) return fail(GBRS_ERR_INVALID, "NULL argument");
    if (m->H < 32)
        for (uint32_t l = 0; l < m->L; ++l)
            if (allowed[l] >> m->H) return fail(GBRS_ERR_INVALID, "allowed[%u] names a haplotype >= num_haps", l);
    GBRS_TRY(select_device(m->device));
    hipStream_t s = m->stream;
    DevBuf<uint32_t> d_allowed;
    GBRS_TRY(d_allowed.alloc(m->L));
    GBRS_HIP_CHECK(hipMemcpyAsync(d_allowed.p, allowed, (size_t)m->L * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    GBRS_TRY(mo_reserve_flags(m));
    for (uint32_t h = 0; h < m->H; ++h) {
        const uint64_t n = m->m.nnz[h];
        MO_LAUNCH(mo_column_flag_kernel, n + 1, s, n, m->m.ip[h].p, m->L, d_allowed.p, h, m->flag.p);
        GBRS_TRY(mo_apply_flags(m, h));
    }
    return GBRS_OK;
}

int gbrs_matops_sizes(gbrs_matops_t *m, uint64_t *num_rows, uint64_t *nnz_per_hap, uint32_t *sorted_inputs) {
    if (!m) return fail(GBRS_ERR_INVALID, "NULL handle");
    if (num_rows) *num_rows = m->R;
    if (nnz_per_hap)
        for (uint32_t h = 0; h < m->H; ++h) nnz_per_hap[h] = m->m.nnz[h];
    if (sorted_inputs) *sorted_inputs = m->sorted_inputs;
    return GBRS_OK;
}

int gbrs_matops_get(gbrs_matops_t *m, uint32_t *const *indptr_out, uint32_t *const *indices_out) {
    RoctxRange roctx_range("gbrs_matops_get");
    if (!m || !indptr_out || !indices_out) return fail(GBRS_ERR_INVALID, "NULL argument");
    GBRS_TRY(select_device(m->device));
    hipStream_t s = m->stream;
    for (uint32_t h = 0; h < m->H; ++h) {
        if (!indptr_out[h] || (m->m.nnz[h] && !indices_out[h]))
            return fail(GBRS_ERR_INVALID, "output array of haplotype %u is NULL", h);
        GBRS_HIP_CHECK(hipMemcpyAsync(indptr_out[h], m->m.ip[h].p, ((size_t)m->L + 1) * sizeof(uint32_t),
                                      hipMemcpyDeviceToHost, s));
        if (m->m.nnz[h])
            GBRS_HIP_CHECK(hipMemcpyAsync(indices_out[h], m->m.ix[h].p, m->m.nnz[h] * sizeof(uint32_t),
                                          hipMemcpyDeviceToHost, s));
    }
    GBRS_HIP_CHECK(hipStreamSynchronize(s));
    return GBRS_OK;
}

int gbrs_matops_shared_counts(gbrs_matops_t *m, const int32_t *locus_group, uint32_t num_groups, uint64_t *nnz_out) {
    RoctxRange roctx_range("gbrs_matops_shared_counts");
    if (!m) return fail(GBRS_ERR_INVALID, "NULL handle");
    const uint32_t L = m->L;
    const uint64_t n_cols = locus_group ? num_groups : L;
    if (locus_group) {
        if (n_cols < 1) return fail(GBRS_ERR_INVALID, "locus_group given with num_groups = 0");
        for (uint32_t l = 0; l < L; ++l)
            if (locus_group[l] < -1 || locus_group[l] >= (int64_t)n_cols)
                return fail(GBRS_ERR_INVALID, "locus_group[%u] = %d is outside [-1, %u)", l, locus_group[l], num_groups);
    }
    uint64_t budget = 0;
    if (std::getenv("GBRS_SHARED_PAIR_BUDGET")) GBRS_TRY(sc_budget(budget));      // a bad value is refused before any work
    GBRS_TRY(select_device(m->device));
    hipStream_t s = m->stream;
    m->sc_valid = false;
    m->sc_keys.release();
    m->sc_cnt.release();
    m->sc_indptr.release();
    const uint32_t cb = bits_for(n_cols - 1);
    ScPeak pm;
    pm.start();
    ScEvents ev;
    GBRS_HIP_CHECK(hipEventCreate(&ev.a));
    GBRS_HIP_CHECK(hipEventCreate(&ev.b));
    GBRS_HIP_CHECK(hipEventRecord(ev.a, s));
    Scratch sc;                                         // this call's own: it goes back when the call ends
    DevBuf<int32_t> group;
    if (locus_group) {
        GBRS_TRY(group.alloc(L));
        GBRS_HIP_CHECK(hipMemcpyAsync(group.p, locus_group, (size_t)L * sizeof(int32_t), hipMemcpyHostToDevice, s));
    }
    DevBuf<uint64_t> pk;
    uint64_t N = 0, T = 0;
    GBRS_TRY(sc_pattern(m, sc, pm, locus_group ? group.p : (const int32_t *)nullptr, cb, pk, N));
    DevBuf<uint64_t> off, d_count;
    GBRS_TRY(d_count.alloc(1));
    if (N) {
        DevBuf<uint64_t> cnt;
        GBRS_TRY(cnt.alloc(N + 1));
        GBRS_TRY(off.alloc(N + 1));
        MO_LAUNCH(sc_pair_count_kernel, N + 1, s, N, pk.p, cb, cnt.p);
        GBRS_TRY(exclusive_scan(sc, cnt.p, off.p, (size_t)N + 1, s));
        pm.sample();
        GBRS_TRY(sc_fetch(off.p + N, T, s));
    }
    if (!budget) GBRS_TRY(sc_budget(budget));
    // the running result: U distinct (i << cb | j) keys, i <= j, ascending, with their counts
    DevBuf<uint64_t> ak;
    DevBuf<uint32_t> ac;
    uint64_t U = 0;
    uint32_t batches = 0;
    if (T) {
        const uint64_t cap = std::min(T, budget);
        DevBuf<uint64_t> ea, eb;
        DevBuf<uint32_t> bc;
        GBRS_TRY(ea.alloc(cap));
        GBRS_TRY(eb.alloc(cap));
        GBRS_TRY(bc.alloc(cap));
        for (uint64_t p0 = 0; p0 < T; p0 += budget, ++batches) {
            const uint64_t c = std::min(budget, T - p0);
            uint64_t nb = 0;
            MO_LAUNCH(sc_emit_kernel, c, s, p0, c, off.p, N, pk.p, cb, ea.p);
            GBRS_TRY(sort_keys64(sc, ea.p, eb.p, c, 2 * cb, s));
            GBRS_TRY(sum_by_key64(sc, eb.p, rocprim::constant_iterator<uint32_t>(1u), ea.p, bc.p, d_count.p, c, s));
            GBRS_TRY(sc_fetch(d_count.p, nb, s));
            DevBuf<uint64_t> mk, sk;
            DevBuf<uint32_t> mc, sv;
            GBRS_TRY(mk.alloc(U + nb));
            GBRS_TRY(mc.alloc(U + nb));
            if (U) {
                GBRS_HIP_CHECK(hipMemcpyAsync(mk.p, ak.p, U * sizeof(uint64_t), hipMemcpyDeviceToDevice, s));
                GBRS_HIP_CHECK(hipMemcpyAsync(mc.p, ac.p, U * sizeof(uint32_t), hipMemcpyDeviceToDevice, s));
            }
            GBRS_HIP_CHECK(hipMemcpyAsync(mk.p + U, ea.p, nb * sizeof(uint64_t), hipMemcpyDeviceToDevice, s));
            GBRS_HIP_CHECK(hipMemcpyAsync(mc.p + U, bc.p, nb * sizeof(uint32_t), hipMemcpyDeviceToDevice, s));
            if (U) {                                    // merge: sort the two sorted runs together, add equal keys up
                GBRS_TRY(sk.alloc(U + nb));
                GBRS_TRY(sv.alloc(U + nb));
                GBRS_TRY(sort_pairs(sc, mk.p, sk.p, mc.p, sv.p, U + nb, 2 * cb, s));
                GBRS_TRY(sum_by_key64(sc, sk.p, sv.p, mk.p, mc.p, d_count.p, U + nb, s));
                pm.sample();
                GBRS_TRY(sc_fetch(d_count.p, U, s));
            } else {
                pm.sample();
                GBRS_HIP_CHECK(hipStreamSynchronize(s));
                U = nb;
            }
            ak.swap(mk);
            ac.swap(mc);
        }
    }
    off.release();
    pk.release();
    // both triangles in CSR order
    uint64_t nnz = 0;
    GBRS_TRY(m->sc_indptr.alloc(n_cols + 1));
    if (U) {
        DevBuf<uint64_t> fk;
        DevBuf<uint32_t> fc;
        GBRS_TRY(fk.alloc(2 * U));
        GBRS_TRY(fc.alloc(2 * U));
        GBRS_TRY(m->sc_keys.alloc(2 * U));
        GBRS_TRY(m->sc_cnt.alloc(2 * U));
        MO_LAUNCH(sc_mirror_kernel, U, s, U, ak.p, ac.p, cb, n_cols, fk.p, fc.p);
        GBRS_TRY(sort_pairs(sc, fk.p, m->sc_keys.p, fc.p, m->sc_cnt.p, 2 * U, cb + bits_for(n_cols), s));
        MO_LAUNCH(sc_indptr_kernel, n_cols + 1, s, n_cols, m->sc_keys.p, 2 * U, cb, m->sc_indptr.p);
        pm.sample();
        GBRS_TRY(sc_fetch(m->sc_indptr.p + n_cols, nnz, s));
    } else {
        GBRS_HIP_CHECK(hipMemsetAsync(m->sc_indptr.p, 0, m->sc_indptr.bytes(), s));
    }
    GBRS_HIP_CHECK(hipEventRecord(ev.b, s));
    GBRS_HIP_CHECK(hipEventSynchronize(ev.b));
    float ms = 0.f;
    GBRS_HIP_CHECK(hipEventElapsedTime(&ms, ev.a, ev.b));
    m->sc_n = n_cols; m->sc_nnz = nnz; m->sc_cb = cb; m->sc_pattern = N; m->sc_pairs = T; m->sc_budget = budget;
    m->sc_batches = batches; m->sc_peak = pm.peak; m->sc_ms = ms;
    m->sc_valid = true;
    if (nnz_out) *nnz_out = nnz;
    return GBRS_OK;
}

int gbrs_matops_shared_counts_get(gbrs_matops_t *m, uint64_t *indptr_out, uint32_t *indices_out, double *data_out) {
    RoctxRange roctx_range("gbrs_matops_shared_counts_get");
    if (!m || !indptr_out) return fail(GBRS_ERR_INVALID, "NULL argument");
    if (!m->sc_valid) return fail(GBRS_ERR_INVALID, "gbrs_matops_shared_counts has not left a result");
    if (m->sc_nnz && (!indices_out || !data_out)) return fail(GBRS_ERR_INVALID, "output array is NULL");
    GBRS_TRY(select_device(m->device));
    hipStream_t s = m->stream;
    const uint64_t nnz = m->sc_nnz;
    GBRS_HIP_CHECK(hipMemcpyAsync(indptr_out, m->sc_indptr.p, (m->sc_n + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    DevBuf<uint32_t> idx;
    DevBuf<double> dat;
    if (nnz) {
        GBRS_TRY(idx.alloc(nnz));
        GBRS_TRY(dat.alloc(nnz));
        MO_LAUNCH(sc_unpack_kernel, nnz, s, nnz, m->sc_keys.p, m->sc_cnt.p, m->sc_cb, idx.p, dat.p);
        GBRS_HIP_CHECK(hipMemcpyAsync(indices_out, idx.p, nnz * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        GBRS_HIP_CHECK(hipMemcpyAsync(data_out, dat.p, nnz * sizeof(double), hipMemcpyDeviceToHost, s));
    }
    GBRS_HIP_CHECK(hipStreamSynchronize(s));
    return GBRS_OK;
}

int gbrs_matops_shared_counts_info(gbrs_matops_t *m, uint64_t *num_columns, uint64_t *pattern_entries,
                                   uint64_t *pairs_emitted, uint32_t *batches, uint64_t *pair_budget,
                                   uint64_t *peak_device_bytes, double *device_ms) {
    if (!m) return fail(GBRS_ERR_INVALID, "NULL handle");
    if (!m->sc_valid) return fail(GBRS_ERR_INVALID, "gbrs_matops_shared_counts has not left a result");
    if (num_columns) *num_columns = m->sc_n;
    if (pattern_entries) *pattern_entries = m->sc_pattern;
    if (pairs_emitted) *pairs_emitted = m->sc_pairs;
    if (batches) *batches = m->sc_batches;
    if (pair_budget) *pair_budget = m->sc_budget;
    if (peak_device_bytes) *peak_device_bytes = m->sc_peak;
    if (device_ms) *device_ms = m->sc_ms;
    return GBRS_OK;
}

int gbrs_matops_destroy(gbrs_matops_t *m) {
    if (!m) return GBRS_OK;
    (void)hipSetDevice(m->device);
    if (m->stream) {
        (void)hipStreamSynchronize(m->stream);
        (void)hipStreamDestroy(m->stream);
    }
    delete m;
    return GBRS_OK;
}

}  // extern "C"
