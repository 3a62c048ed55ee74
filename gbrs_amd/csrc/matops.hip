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
