// Row sharding of one sample's CSC arrays on the device (`gbrs quantify --gpus N`, gbrs_amd/sharded.py), included at
// the end of em_layout.hip for its rocPRIM scan helpers.  The three calls reproduce gbrs_amd.dist.shard_rows exactly:
//   plan    per-row entry histogram (integer atomics: the same counts in any order), a 64-bit inclusive scan and one
//           binary search per bound with numpy's searchsorted(cum, total * k / world, 'left') comparison in float64
//   index   per haplotype: keep flag of every entry (r0 <= row < r1), an exclusive scan of the flags; the local column
//           pointer of locus l is the scan at the column's first entry, so a column of any length is as parallel as
//           the rest and the kept entries keep their order inside it
//   gather  the same scan, then every kept entry is scattered to its position with its row id re-based to r0 (and
//           its stored value); with l_split > 0 every local row also notes the side(s) of the cut its entries lie
//           on, and the rows that have both are counted
// Every row id is compared with num_rows before anything is indexed with it, and every column pointer is checked
// before the scan is read at it: a bad input returns GBRS_ERR_INVALID.

namespace gbrs {
namespace {

constexpr unsigned SHARD_BLOCK = 256;

inline unsigned shard_grid(uint64_t n) {
    const uint64_t g = (n + SHARD_BLOCK - 1) / SHARD_BLOCK;
    return (unsigned)std::min<uint64_t>(std::max<uint64_t>(g, 1), 65536);
}

// indptr[0] == 0, non-decreasing, indptr[L] == nnz (the caller read nnz from indptr[L])
__global__ void __launch_bounds__(SHARD_BLOCK)
shard_check_indptr_kernel(uint32_t L, const uint32_t *__restrict__ ip, uint32_t *__restrict__ bad) {
    for (uint64_t l = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; l <= L; l += (uint64_t)gridDim.x * blockDim.x) {
        const bool ok = l == 0 ? ip[0] == 0u : ip[l - 1] <= ip[l];
        if (!ok) atomicOr(bad, 1u);
    }
}

__global__ void __launch_bounds__(SHARD_BLOCK)
shard_row_hist_kernel(uint64_t n, const uint32_t *__restrict__ ix, uint64_t R, unsigned long long *__restrict__ per_row,
                      uint32_t *__restrict__ bad) {
    for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t r = ix[k];
        if (r < R) atomicAdd(&per_row[r], 1ull);
        else atomicOr(bad, 2u);
    }
}

// bounds[k] for 0 < k < world: searchsorted([0, incl...], total * k / world, 'left') with numpy's float64 comparison
__global__ void __launch_bounds__(64)
shard_bounds_kernel(uint64_t R, const uint64_t *__restrict__ incl, int world, uint64_t *__restrict__ bounds) {
    const int k = (int)threadIdx.x + 1;
    if (k >= world) return;
    const uint64_t total = incl[R - 1];
    const double target = (double)(int64_t)(total * (uint64_t)k) / (double)world;
    uint64_t b = 0;
    if (target > 0.0) {
        uint64_t lo = 0, hi = R;              // first j with (double)incl[j] >= target
        while (lo < hi) {
            const uint64_t mid = lo + (hi - lo) / 2;
            if ((double)incl[mid] >= target) hi = mid;
            else lo = mid + 1;
        }
        b = lo + 1;                           // cum = [0, incl...]: index j of incl is index j + 1 of cum
    }
    bounds[k] = b;
}

// flag[k] = (r0 <= ix[k] < r1); flag[n] = 0 so that the exclusive scan's last element is the kept count
__global__ void __launch_bounds__(SHARD_BLOCK)
shard_flag_kernel(uint64_t n, const uint32_t *__restrict__ ix, uint64_t R, uint64_t r0, uint64_t r1,
                  uint32_t *__restrict__ flag, uint32_t *__restrict__ bad) {
    for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k <= n; k += (uint64_t)gridDim.x * blockDim.x) {
        uint32_t f = 0;
        if (k < n) {
            const uint32_t r = ix[k];
            if (r >= R) atomicOr(bad, 2u);
            f = (r >= r0 && r < r1) ? 1u : 0u;
        }
        flag[k] = f;
    }
}

__global__ void __launch_bounds__(SHARD_BLOCK)
shard_indptr_kernel(uint32_t L, const uint32_t *__restrict__ ip, const uint32_t *__restrict__ pos,
                    uint32_t *__restrict__ ip_out) {
    for (uint64_t l = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; l <= L; l += (uint64_t)gridDim.x * blockDim.x)
        ip_out[l] = pos[ip[l]];
}

// side bits per local row: 1 = an entry left of the cut (entry index < cut), 2 = right of it
__global__ void __launch_bounds__(SHARD_BLOCK)
shard_scatter_kernel(uint64_t n, const uint32_t *__restrict__ ix, const double *__restrict__ val, uint64_t r0,
                     uint64_t r1, const uint32_t *__restrict__ flag, const uint32_t *__restrict__ pos,
                     uint32_t *__restrict__ ix_out, double *__restrict__ val_out, uint64_t cut,
                     uint32_t *__restrict__ side) {
    for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (uint64_t)gridDim.x * blockDim.x) {
        if (!flag[k]) continue;
        const uint32_t o = pos[k];
        const uint32_t local = (uint32_t)(ix[k] - r0);
        ix_out[o] = local;
        if (val) val_out[o] = val[k];
        if (side) atomicOr(&side[local], k < cut ? 1u : 2u);
    }
}

__global__ void __launch_bounds__(SHARD_BLOCK)
shard_straddle_kernel(uint64_t n, const uint32_t *__restrict__ side, unsigned long long *__restrict__ count) {
    unsigned long long c = 0;
    for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k - (threadIdx.x & 63) < n;
         k += (uint64_t)gridDim.x * blockDim.x) {
        const bool both = k < n && side[k] == 3u;
        c += __popcll(__ballot(both));        // 64-bit ballot: one bit per lane of the wavefront
    }
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(count, c);
}

struct ShardStream {
    hipStream_t s = nullptr;
    ~ShardStream() {
        if (s) {
            (void)hipStreamSynchronize(s);
            (void)hipStreamDestroy(s);
        }
    }
};

int shard_args(uint64_t R, uint32_t L, uint32_t H, const uint32_t *const *indptr, const uint32_t *const *indices,
               int device) {
    if (H < 1 || H > 32 || L < 1 || R < 1 || R > 0xFFFFFFFFull)
        return fail(GBRS_ERR_INVALID, "The shape must be a tuple of three positive integers (H <= 32, R < 2^32).");
    if (!indptr || !indices) return fail(GBRS_ERR_INVALID, "indptr/indices tables are NULL");
    for (uint32_t h = 0; h < H; ++h)
        if (!indptr[h]) return fail(GBRS_ERR_INVALID, "indptr[%u] is NULL", h);
    return select_device(device);
}

// nnz[h] = indptr[h][L], after checking every column pointer table; bad entries of indices are the caller's to check
int shard_nnz(uint32_t L, uint32_t H, const uint32_t *const *indptr, const uint32_t *const *indices,
              std::vector<uint64_t> &nnz, DevBuf<uint32_t> &bad, hipStream_t s) {
    nnz.assign(H, 0);
    std::vector<uint32_t> last(H);
    for (uint32_t h = 0; h < H; ++h) {
        GBRS_HIP_CHECK(hipMemcpyAsync(&last[h], indptr[h] + L, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
        hipLaunchKernelGGL(shard_check_indptr_kernel, dim3(shard_grid((uint64_t)L + 1)), dim3(SHARD_BLOCK), 0, s, L,
                           indptr[h], bad.p);
        GBRS_HIP_CHECK(hipGetLastError());
    }
    uint32_t b = 0;
    GBRS_HIP_CHECK(hipMemcpyAsync(&b, bad.p, sizeof(b), hipMemcpyDeviceToHost, s));
    GBRS_HIP_CHECK(hipStreamSynchronize(s));
    if (b) return fail(GBRS_ERR_INVALID, "Malformed CSC arrays: a column pointer table is not non-decreasing from 0.");
    for (uint32_t h = 0; h < H; ++h) {
        nnz[h] = last[h];
        if (nnz[h] && !indices[h]) return fail(GBRS_ERR_INVALID, "indices[%u] is NULL", h);
    }
    return GBRS_OK;
}

// flags + exclusive scan of haplotype h's entries for rows [r0, r1): pos[k] = kept entries before k, pos[nnz] = all
int shard_scan(Scratch &sc, uint64_t n, const uint32_t *ix, uint64_t R, uint64_t r0, uint64_t r1, DevBuf<uint32_t> &flag,
               DevBuf<uint32_t> &pos, DevBuf<uint32_t> &bad, uint64_t &kept, hipStream_t s) {
    hipLaunchKernelGGL(shard_flag_kernel, dim3(shard_grid(n + 1)), dim3(SHARD_BLOCK), 0, s, n, ix, R, r0, r1, flag.p,
                       bad.p);
    GBRS_HIP_CHECK(hipGetLastError());
    uint32_t b = 0;
    GBRS_HIP_CHECK(hipMemcpyAsync(&b, bad.p, sizeof(b), hipMemcpyDeviceToHost, s));
    GBRS_HIP_CHECK(hipStreamSynchronize(s));
    if (b) return fail(GBRS_ERR_INVALID, "indices hold a row id >= num_rows");
    GBRS_TRY(exclusive_scan(sc, flag.p, pos.p, n + 1, s));
    uint32_t k = 0;
    GBRS_HIP_CHECK(hipMemcpyAsync(&k, pos.p + n, sizeof(k), hipMemcpyDeviceToHost, s));
    GBRS_HIP_CHECK(hipStreamSynchronize(s));
    kept = k;
    return GBRS_OK;
}

int shard_block_args(uint64_t R, uint64_t r0, uint64_t r1) {
    if (r0 > r1 || r1 > R) return fail(GBRS_ERR_INVALID, "row block [%llu, %llu) is not inside [0, %llu)",
                                       (unsigned long long)r0, (unsigned long long)r1, (unsigned long long)R);
    return GBRS_OK;
}

}  // namespace
}  // namespace gbrs

extern "C" {

int gbrs_shard_plan(uint64_t num_rows, uint32_t num_loci, uint32_t num_haps, const uint32_t *const *indptr,
                    const uint32_t *const *indices, int world, int device, uint64_t *bounds) {
    using namespace gbrs;
    RoctxRange roctx_range("gbrs_shard_plan");
    if (!bounds) return fail(GBRS_ERR_INVALID, "bounds is NULL");
    if (world < 1 || world > 64) return fail(GBRS_ERR_INVALID, "world must be 1..64, got %d", world);
    GBRS_TRY(shard_args(num_rows, num_loci, num_haps, indptr, indices, device));
    const uint64_t R = num_rows;
    ShardStream st;
    GBRS_HIP_CHECK(hipStreamCreateWithFlags(&st.s, hipStreamNonBlocking));
    hipStream_t s = st.s;
    DevBuf<uint32_t> bad;
    GBRS_TRY(bad.alloc(1));
    GBRS_HIP_CHECK(hipMemsetAsync(bad.p, 0, sizeof(uint32_t), s));
    std::vector<uint64_t> nnz;
    GBRS_TRY(shard_nnz(num_loci, num_haps, indptr, indices, nnz, bad, s));
    DevBuf<unsigned long long> per_row;
    DevBuf<uint64_t> incl, d_bounds;
    GBRS_TRY(per_row.alloc(R));
    GBRS_TRY(incl.alloc(R));
    GBRS_TRY(d_bounds.alloc((size_t)world + 1));
    GBRS_HIP_CHECK(hipMemsetAsync(per_row.p, 0, per_row.bytes(), s));
    GBRS_HIP_CHECK(hipMemsetAsync(d_bounds.p, 0, d_bounds.bytes(), s));
    for (uint32_t h = 0; h < num_haps; ++h) {
        if (!nnz[h]) continue;
        hipLaunchKernelGGL(shard_row_hist_kernel, dim3(shard_grid(nnz[h])), dim3(SHARD_BLOCK), 0, s, nnz[h], indices[h],
                           R, per_row.p, bad.p);
        GBRS_HIP_CHECK(hipGetLastError());
    }
    uint32_t b = 0;
    GBRS_HIP_CHECK(hipMemcpyAsync(&b, bad.p, sizeof(b), hipMemcpyDeviceToHost, s));
    GBRS_HIP_CHECK(hipStreamSynchronize(s));
    if (b) return fail(GBRS_ERR_INVALID, "indices hold a row id >= num_rows");
    Scratch sc;
    GBRS_TRY(inclusive_scan(sc, reinterpret_cast<const uint64_t *>(per_row.p), incl.p, R, s));
    hipLaunchKernelGGL(shard_bounds_kernel, dim3(1), dim3(64), 0, s, R, incl.p, world, d_bounds.p);
    GBRS_HIP_CHECK(hipGetLastError());
    GBRS_HIP_CHECK(hipMemcpyAsync(bounds, d_bounds.p, ((size_t)world + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    GBRS_HIP_CHECK(hipStreamSynchronize(s));
    bounds[0] = 0;
    bounds[world] = R;
    return GBRS_OK;
}

int gbrs_shard_index(uint64_t num_rows, uint32_t num_loci, uint32_t num_haps, const uint32_t *const *indptr,
                     const uint32_t *const *indices, uint64_t r0, uint64_t r1, int device,
                     uint32_t *const *indptr_out, uint64_t *nnz_out) {
    using namespace gbrs;
    RoctxRange roctx_range("gbrs_shard_index");
    if (!indptr_out || !nnz_out) return fail(GBRS_ERR_INVALID, "indptr_out / nnz_out is NULL");
    GBRS_TRY(shard_args(num_rows, num_loci, num_haps, indptr, indices, device));
    GBRS_TRY(shard_block_args(num_rows, r0, r1));
    for (uint32_t h = 0; h < num_haps; ++h)
        if (!indptr_out[h]) return fail(GBRS_ERR_INVALID, "indptr_out[%u] is NULL", h);
    ShardStream st;
    GBRS_HIP_CHECK(hipStreamCreateWithFlags(&st.s, hipStreamNonBlocking));
    hipStream_t s = st.s;
    DevBuf<uint32_t> bad, flag, pos;
    GBRS_TRY(bad.alloc(1));
    GBRS_HIP_CHECK(hipMemsetAsync(bad.p, 0, sizeof(uint32_t), s));
    std::vector<uint64_t> nnz;
    GBRS_TRY(shard_nnz(num_loci, num_haps, indptr, indices, nnz, bad, s));
    const uint64_t nmax = *std::max_element(nnz.begin(), nnz.end());
    GBRS_TRY(flag.alloc(nmax + 1));
    GBRS_TRY(pos.alloc(nmax + 1));
    Scratch sc;
    for (uint32_t h = 0; h < num_haps; ++h) {
        uint64_t kept = 0;
        GBRS_TRY(shard_scan(sc, nnz[h], indices[h], num_rows, r0, r1, flag, pos, bad, kept, s));
        hipLaunchKernelGGL(shard_indptr_kernel, dim3(shard_grid((uint64_t)num_loci + 1)), dim3(SHARD_BLOCK), 0, s,
                           num_loci, indptr[h], pos.p, indptr_out[h]);
        GBRS_HIP_CHECK(hipGetLastError());
        nnz_out[h] = kept;
    }
    GBRS_HIP_CHECK(hipStreamSynchronize(s));
    return GBRS_OK;
}

int gbrs_shard_gather(uint64_t num_rows, uint32_t num_loci, uint32_t num_haps, const uint32_t *const *indptr,
                      const uint32_t *const *indices, uint64_t r0, uint64_t r1, uint32_t l_split,
                      const double *const *values, int device, const uint64_t *nnz_local,
                      uint32_t *const *indices_out, double *const *values_out, uint64_t *straddling) {
    using namespace gbrs;
    RoctxRange roctx_range("gbrs_shard_gather");
    if (!indices_out || !nnz_local) return fail(GBRS_ERR_INVALID, "indices_out / nnz_local is NULL");
    if (values && !values_out) return fail(GBRS_ERR_INVALID, "values given without values_out");
    if (l_split && !straddling) return fail(GBRS_ERR_INVALID, "l_split given without straddling");
    if (l_split >= num_loci && l_split) return fail(GBRS_ERR_INVALID, "l_split %u not inside (0, %u)", l_split, num_loci);
    GBRS_TRY(shard_args(num_rows, num_loci, num_haps, indptr, indices, device));
    GBRS_TRY(shard_block_args(num_rows, r0, r1));
    ShardStream st;
    GBRS_HIP_CHECK(hipStreamCreateWithFlags(&st.s, hipStreamNonBlocking));
    hipStream_t s = st.s;
    DevBuf<uint32_t> bad, flag, pos, side;
    DevBuf<unsigned long long> d_straddle;
    GBRS_TRY(bad.alloc(1));
    GBRS_HIP_CHECK(hipMemsetAsync(bad.p, 0, sizeof(uint32_t), s));
    std::vector<uint64_t> nnz;
    GBRS_TRY(shard_nnz(num_loci, num_haps, indptr, indices, nnz, bad, s));
    const uint64_t nmax = *std::max_element(nnz.begin(), nnz.end());
    GBRS_TRY(flag.alloc(nmax + 1));
    GBRS_TRY(pos.alloc(nmax + 1));
    const uint64_t R_local = r1 - r0;
    if (l_split) {
        GBRS_TRY(side.alloc(std::max<uint64_t>(R_local, 1)));
        GBRS_TRY(d_straddle.alloc(1));
        GBRS_HIP_CHECK(hipMemsetAsync(side.p, 0, side.bytes(), s));
        GBRS_HIP_CHECK(hipMemsetAsync(d_straddle.p, 0, d_straddle.bytes(), s));
    }
    Scratch sc;
    for (uint32_t h = 0; h < num_haps; ++h) {
        uint64_t kept = 0;
        GBRS_TRY(shard_scan(sc, nnz[h], indices[h], num_rows, r0, r1, flag, pos, bad, kept, s));
        if (kept != nnz_local[h])
            return fail(GBRS_ERR_INVALID, "haplotype %u keeps %llu entries of rows [%llu, %llu), nnz_local says %llu", h,
                        (unsigned long long)kept, (unsigned long long)r0, (unsigned long long)r1,
                        (unsigned long long)nnz_local[h]);
        if (!kept) continue;
        if (!indices_out[h] || (values && (!values[h] || !values_out[h])))
            return fail(GBRS_ERR_INVALID, "output or value array of haplotype %u is NULL", h);
        uint32_t cut = 0;
        if (l_split)
            GBRS_HIP_CHECK(hipMemcpyAsync(&cut, indptr[h] + l_split, sizeof(cut), hipMemcpyDeviceToHost, s));
        GBRS_HIP_CHECK(hipStreamSynchronize(s));
        hipLaunchKernelGGL(shard_scatter_kernel, dim3(shard_grid(nnz[h])), dim3(SHARD_BLOCK), 0, s, nnz[h], indices[h],
                           values ? values[h] : nullptr, r0, r1, flag.p, pos.p, indices_out[h],
                           values ? values_out[h] : nullptr, (uint64_t)cut, l_split ? side.p : nullptr);
        GBRS_HIP_CHECK(hipGetLastError());
    }
    if (l_split) {
        unsigned long long n = 0;
        if (R_local) {
            hipLaunchKernelGGL(shard_straddle_kernel, dim3(shard_grid(R_local)), dim3(SHARD_BLOCK), 0, s, R_local,
                               side.p, d_straddle.p);
            GBRS_HIP_CHECK(hipGetLastError());
            GBRS_HIP_CHECK(hipMemcpyAsync(&n, d_straddle.p, sizeof(n), hipMemcpyDeviceToHost, s));
        }
        GBRS_HIP_CHECK(hipStreamSynchronize(s));
        *straddling = n;
    }
    GBRS_HIP_CHECK(hipStreamSynchronize(s));
    return GBRS_OK;
}

}  // extern "C"
