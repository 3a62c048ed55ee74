// gbrs_tensor_*: the value-carrying alignment tensor and the arithmetic the reference builds its models from
// (emase/Sparse3DMatrix.py reset / multiply / copy, emase/AlignmentPropertyMatrix.py normalize_reads / sum).
//
// A handle is a value array on a structure.  The structure (CSC row ids and column offsets, row offsets, count, genes and
// the grouped row orders) is fixed after create and shared by reference count between a handle and its copies; a handle
// owns its float64 values and its `eliminated` bytes, both in CSC order (column c = h*L + l).
//
//   elementwise   one lane per CSC entry: reset and the five multiply forms.  The column of an entry comes from
//                 entry_column (em_layout.h), haplotype and locus from the column, the read from ent_row.
//   row pass      one lane per read walks its entries in a grouped order (em_layout.hip build_grouped_order): the sum of a
//                 run - the read, a locus, a gene, a gene x haplotype - then val[src[j]] /= sum over the same run.  The
//                 per-haplotype runs of normalize_reads(HAPLOTYPE) and sum(LOCUS) are not contiguous in any gene-major
//                 order, so they keep one accumulator per haplotype in registers instead.
//   sum(READ)     the CSC entries in order, val * count[read]: a wavefront that sits in one column adds up first and
//                 issues one atomic, otherwise one atomic per lane (as model_col_kernel, em_models.inc).
//
// An entry whose value is 0 when normalize_reads(LOCUS | GROUP | HAPLOGROUP) runs is eliminated: it keeps 0 through every
// later operation, reset included (the reference drops it from its sparse structure there).  A live entry over a zero
// denominator sets the handle's error flag and is left alone; the call then returns GBRS_ERR_FLOAT.
//
// Every operation but sum(READ) is free of float atomics and adds in the fixed order of the layout: bit-identical from run
// to run.  sum(READ) adds with float atomics in global memory, so its last bits depend on the order the wavefronts arrive.
#include "em_layout.h"
#include "prim.h"

#include <algorithm>
#include <memory>

using namespace gbrs;

namespace {

enum Form : int { FORM_RESET = 0, FORM_LOCUS = 1, FORM_READ = 2, FORM_READ_HAP = 3, FORM_HAP_LOCUS = 4, FORM_TENSOR = 5 };
enum Axis : int { AX_LOCUS = 0, AX_HAPLOTYPE = 1, AX_READ = 2, AX_GROUP = 3, AX_HAPLOGROUP = 4 };

struct TensorStructure {
    int device = 0;
    uint64_t R = 0, N = 0;
    uint32_t L = 0, H = 0;
    bool has_count = false;
    std::vector<uint64_t> hap_off;      // H + 1: first entry of every haplotype
    DevBuf<uint32_t> ent_row;           // N
    DevBuf<uint64_t> col_ptr;           // H*L + 1
    DevBuf<uint32_t> row_ptr;           // R + 1
    DevBuf<double> count;               // R
    DevBuf<uint32_t> locus_gene;        // L
    DevBuf<uint32_t> rank_lh, inv_lh;   // (row, gene, locus, haplotype): column -> rank, rank -> l*32 + h
    DevBuf<uint32_t> rank_hl, inv_hl;   // (row, gene, haplotype, locus)
    GroupedOrder order_lh, order_hl;    // built at the first row-wise / the first HAPLOGROUP call
    DevBuf<double> mult;                // the multiplier of the call in flight
    DevBuf<double> acc;                 // H*L: sum(READ)
    DevBuf<double> rows_out;            // R*H: sum(LOCUS)
    DevBuf<unsigned long long> nnz;     // H
    DevBuf<int> flag;                   // float error of the call in flight
    hipStream_t stream = nullptr;
    ~TensorStructure() {
        if (stream) (void)hipStreamDestroy(stream);
    }
};

}  // namespace

struct gbrs_tensor {
    std::shared_ptr<TensorStructure> st;
    DevBuf<double> val;                 // N
    DevBuf<uint8_t> elim;               // N: 1 = eliminated
};

namespace {

// ---- kernels -----------------------------------------------------------------------------------------------------

template <int FORM>
__global__ void __launch_bounds__(256)
tensor_elementwise_kernel(uint64_t n, uint32_t ncols, uint32_t L, uint32_t H,
                          const uint64_t *__restrict__ col_ptr, const uint32_t *__restrict__ ent_row,
                          const uint8_t *__restrict__ elim, const double *m /* may be val itself */, double *val) {
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k - (threadIdx.x & 63) >= n) return;
    const bool in_range = k < n;
    uint32_t c = 0;
    if (FORM == FORM_LOCUS || FORM == FORM_READ_HAP || FORM == FORM_HAP_LOCUS)      // (the whole wavefront searches together)
        c = entry_column(col_ptr, ncols, in_range ? k : n - 1, n);
    if (!in_range || elim[k]) return;
    if (FORM == FORM_RESET) {
        val[k] = 1.0;
        return;
    }
    const uint32_t h = c / L, l = c - h * L;
    const double f = FORM == FORM_LOCUS      ? m[l]
                     : FORM == FORM_READ     ? m[ent_row[k]]
                     : FORM == FORM_READ_HAP ? m[(size_t)ent_row[k] * H + h]
                     : FORM == FORM_HAP_LOCUS ? m[c]
                                              : m[k];                               // FORM_TENSOR: the other handle's values
    val[k] *= f;
}

template <int AXIS>
__device__ __forceinline__ uint32_t run_key(uint32_t w, const uint32_t *__restrict__ locus_gene) {
    return AXIS == AX_READ ? 0u : AXIS == AX_LOCUS ? (w >> 5) : AXIS == AX_GROUP ? locus_gene[w >> 5]
                                                                                : locus_gene[w >> 5] * 32u + (w & 31u);
}

// READ, LOCUS, GROUP on the (row, gene, locus, haplotype) order, HAPLOGROUP on (row, gene, haplotype, locus): the runs of
// the axis are contiguous.  L < 2^27, so gene * 32 + h fits 32 bits.
template <int AXIS>
__global__ void __launch_bounds__(256)
tensor_normalize_kernel(uint64_t R, const uint32_t *__restrict__ row_ptr, const uint32_t *__restrict__ lh,
                        const uint32_t *__restrict__ src, const uint32_t *__restrict__ locus_gene,
                        double *__restrict__ val, uint8_t *__restrict__ elim, int *__restrict__ flag) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= R) return;
    const uint32_t a = row_ptr[r], b = row_ptr[r + 1];
    if (AXIS != AX_READ)                                   // eliminate_zeros() before the division
        for (uint32_t j = a; j < b; ++j)
            if (val[src[j]] == 0.0) elim[src[j]] = 1;
    for (uint32_t p = a; p < b;) {
        const uint32_t key = run_key<AXIS>(lh[p], locus_gene);
        double sum = 0.0;
        bool any_live = false;
        uint32_t q = p;
        for (; q < b && run_key<AXIS>(lh[q], locus_gene) == key; ++q) {
            sum += val[src[q]];                            // (an eliminated entry holds 0)
            any_live |= !elim[src[q]];
        }
        if (sum == 0.0) {                                  // the entries stay as they are
            if (any_live) *flag = 1;
        } else
            for (uint32_t j = p; j < q; ++j)
                if (!elim[src[j]]) val[src[j]] /= sum;
        p = q;
    }
}

template <int HT>
__device__ __forceinline__ double pick(const double (&acc)[HT], uint32_t h) {
    double r = 0.0;
#pragma unroll
    for (int t = 0; t < HT; ++t) r = (uint32_t)t == h ? acc[t] : r;
    return r;
}

// the per-haplotype sums of a read over all its loci: out (R x H, nullable) receives them, and with `divide` every live
// entry is divided by the sum of its haplotype (DIVIDE: normalize_reads(HAPLOTYPE)).  HT >= H accumulators, statically indexed.
template <int HT, bool DIVIDE>
__global__ void __launch_bounds__(256)
tensor_hap_sums_kernel(uint64_t R, uint32_t H, const uint32_t *__restrict__ row_ptr, const uint32_t *__restrict__ lh,
                       const uint32_t *__restrict__ src, double *__restrict__ val, const uint8_t *__restrict__ elim,
                       double *__restrict__ out, int *__restrict__ flag) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= R) return;
    const uint32_t a = row_ptr[r], b = row_ptr[r + 1];
    double acc[HT];
    uint32_t live = 0;                                     // bit h: the read has a live entry of haplotype h
#pragma unroll
    for (int t = 0; t < HT; ++t) acc[t] = 0.0;
    for (uint32_t j = a; j < b; ++j) {
        const uint32_t h = lh[j] & 31u, k = src[j];
        const double v = val[k];
#pragma unroll
        for (int t = 0; t < HT; ++t) acc[t] += (uint32_t)t == h ? v : 0.0;
        live |= elim[k] ? 0u : 1u << h;
    }
    if (out)
#pragma unroll
        for (int t = 0; t < HT; ++t)
            if ((uint32_t)t < H) out[r * H + t] = acc[t];
    if (!DIVIDE) return;
    uint32_t bad = 0;
#pragma unroll
    for (int t = 0; t < HT; ++t) bad |= acc[t] == 0.0 ? 1u << t : 0u;
    if (live & bad) *flag = 1;
    for (uint32_t j = a; j < b; ++j) {
        const uint32_t h = lh[j] & 31u, k = src[j];
        if (elim[k] || ((bad >> h) & 1u)) continue;
        val[k] /= pick<HT>(acc, h);
    }
}

// acc is (H x L) row-major: element h*L + l is the column id itself
__global__ void __launch_bounds__(256)
tensor_sum_reads_kernel(uint64_t n, uint32_t ncols, const uint64_t *__restrict__ col_ptr,
                        const uint32_t *__restrict__ ent_row, const double *__restrict__ val,
                        const double *__restrict__ count, double *__restrict__ acc) {
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k - (threadIdx.x & 63) >= n) return;
    const bool in_range = k < n;
    const uint32_t c = entry_column(col_ptr, ncols, in_range ? k : n - 1, n);
    const double w = in_range ? (count ? val[k] * count[ent_row[k]] : val[k]) : 0.0;
    const uint32_t c0 = __shfl(c, 0, WAVE);
    if (__all(c == c0)) {
        const double s = wave_sum(w);
        if ((threadIdx.x & 63) == 0) atomicAdd(&acc[c0], s);
    } else if (in_range) {
        atomicAdd(&acc[c], w);
    }
}

__global__ void __launch_bounds__(256)
tensor_count_live_kernel(uint64_t first, uint64_t end, const uint8_t *__restrict__ elim, unsigned long long *__restrict__ out) {
    const uint64_t k = first + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const unsigned long long live = __ballot(k < end && !elim[k]);
    if ((threadIdx.x & 63) == 0 && live) atomicAdd(out, (unsigned long long)__popcll(live));
}

__global__ void __launch_bounds__(256)
tensor_clear_eliminated_kernel(uint64_t first, uint64_t end, const uint8_t *__restrict__ elim, double *__restrict__ val) {
    const uint64_t k = first + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k < end && elim[k]) val[k] = 0.0;
}

// ---- host --------------------------------------------------------------------------------------------------------

int check_handle(const gbrs_tensor *t) {
    if (!t) return fail(GBRS_ERR_INVALID, "handle is NULL");
    if (!t->st) return fail(GBRS_ERR_STATE, "the tensor handle holds no structure");
    return select_device(t->st->device);
}

int upload_u32(DevBuf<uint32_t> &d, const std::vector<uint32_t> &v, hipStream_t s) {
    GBRS_TRY(d.alloc(std::max<size_t>(v.size(), 1)));
    if (!v.empty()) GBRS_HIP_CHECK(hipMemcpyAsync(d.p, v.data(), v.size() * 4, hipMemcpyHostToDevice, s));
    return GBRS_OK;
}

// genes: the groups in order, then every locus in no group as a gene of its own (gbrs_em_set_groups, em.hip)
int set_groups_impl(TensorStructure &st, int64_t G, const int64_t *group_ptr, const int64_t *members) {
    const uint32_t L = st.L, H = st.H;
    if (G > 0 && group_ptr[0] != 0) return fail(GBRS_ERR_INVALID, "group_ptr[0] != 0");
    for (int64_t g = 0; g < G; ++g)
        if (group_ptr[g + 1] < group_ptr[g]) return fail(GBRS_ERR_INVALID, "group_ptr not monotone");
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
    std::vector<uint32_t> gptr{0}, lgene(L), pos(L);
    uint32_t n_mem = 0;
    for (int64_t g = 0; g < G; ++g) {
        std::sort(mem[g].begin(), mem[g].end());
        for (uint32_t l : mem[g]) { lgene[l] = (uint32_t)(gptr.size() - 1); pos[l] = n_mem++; }
        gptr.push_back(n_mem);
    }
    for (uint32_t l = 0; l < L; ++l)
        if (gene[l] < 0) { lgene[l] = (uint32_t)(gptr.size() - 1); pos[l] = n_mem++; gptr.push_back(n_mem); }
    const size_t HL = (size_t)H * L;
    std::vector<uint32_t> r_lh(HL), i_lh(HL), r_hl(HL), i_hl(HL);
    for (uint32_t l = 0; l < L; ++l) {
        const uint32_t g = lgene[l], start = gptr[g], size = gptr[g + 1] - start;
        for (uint32_t h = 0; h < H; ++h) {
            const uint32_t a = pos[l] * H + h, b = start * H + h * size + (pos[l] - start);
            r_lh[(size_t)h * L + l] = a;
            i_lh[a] = l * 32u + h;
            r_hl[(size_t)h * L + l] = b;
            i_hl[b] = l * 32u + h;
        }
    }
    st.order_lh.built = st.order_hl.built = false;
    GBRS_TRY(upload_u32(st.locus_gene, lgene, st.stream));
    GBRS_TRY(upload_u32(st.rank_lh, r_lh, st.stream));
    GBRS_TRY(upload_u32(st.inv_lh, i_lh, st.stream));
    GBRS_TRY(upload_u32(st.rank_hl, r_hl, st.stream));
    GBRS_TRY(upload_u32(st.inv_hl, i_hl, st.stream));
    GBRS_HIP_CHECK(hipStreamSynchronize(st.stream));       // (the host vectors go out of scope)
    return GBRS_OK;
}

int ensure_order(TensorStructure &st, bool hap_major) {
    GroupedOrder &o = hap_major ? st.order_hl : st.order_lh;
    if (o.built) return GBRS_OK;
    return build_grouped_order(o, st.R, st.L, st.H, st.N, st.ent_row.p, st.col_ptr.p,
                               hap_major ? st.rank_hl.p : st.rank_lh.p, hap_major ? st.inv_hl.p : st.inv_lh.p, st.stream);
}

int clear_flag(TensorStructure &st) {
    GBRS_HIP_CHECK(hipMemsetAsync(st.flag.p, 0, sizeof(int), st.stream));
    return GBRS_OK;
}

// as em_check_float (em.hip): the flag of the call that just ran, read back at the call
int check_float(TensorStructure &st) {
    int host = 0;
    GBRS_HIP_CHECK(hipGetLastError());
    GBRS_HIP_CHECK(hipMemcpyAsync(&host, st.flag.p, sizeof(int), hipMemcpyDeviceToHost, st.stream));
    GBRS_HIP_CHECK(hipStreamSynchronize(st.stream));
    if (host)
        return fail(GBRS_ERR_FLOAT, "invalid value encountered in divide (a read's alignments add up to zero along the axis)");
    return GBRS_OK;
}

int launch_elementwise(gbrs_tensor *t, int form, const double *m) {
    TensorStructure &st = *t->st;
    if (st.N == 0) return GBRS_OK;
#define GBRS_LAUNCH_ELEMENTWISE(F)                                                                                     \
    case F:                                                                                                            \
        hipLaunchKernelGGL(tensor_elementwise_kernel<F>, dim3(grid_for(st.N)), dim3(256), 0, st.stream, st.N,          \
                           st.H * st.L, st.L, st.H, st.col_ptr.p, st.ent_row.p, t->elim.p, m, t->val.p);               \
        break
    switch (form) {
        GBRS_LAUNCH_ELEMENTWISE(FORM_RESET);
        GBRS_LAUNCH_ELEMENTWISE(FORM_LOCUS);
        GBRS_LAUNCH_ELEMENTWISE(FORM_READ);
        GBRS_LAUNCH_ELEMENTWISE(FORM_READ_HAP);
        GBRS_LAUNCH_ELEMENTWISE(FORM_HAP_LOCUS);
        GBRS_LAUNCH_ELEMENTWISE(FORM_TENSOR);
    default: return fail(GBRS_ERR_INVALID, "multiply form %d", form);
    }
#undef GBRS_LAUNCH_ELEMENTWISE
    GBRS_HIP_CHECK(hipGetLastError());
    GBRS_HIP_CHECK(hipStreamSynchronize(st.stream));
    return GBRS_OK;
}

template <int HT>
void launch_hap_sums(gbrs_tensor *t, double *out, bool divide) {
    TensorStructure &st = *t->st;
    const dim3 grid(grid_for(st.R)), block(256);
    if (divide)
        hipLaunchKernelGGL((tensor_hap_sums_kernel<HT, true>), grid, block, 0, st.stream, st.R, st.H, st.row_ptr.p,
                           st.order_lh.lh.p, st.order_lh.src.p, t->val.p, t->elim.p, out, st.flag.p);
    else
        hipLaunchKernelGGL((tensor_hap_sums_kernel<HT, false>), grid, block, 0, st.stream, st.R, st.H, st.row_ptr.p,
                           st.order_lh.lh.p, st.order_lh.src.p, t->val.p, t->elim.p, out, st.flag.p);
}

void dispatch_hap_sums(gbrs_tensor *t, double *out, bool divide) {
    const uint32_t H = t->st->H;
    if (H <= 1) launch_hap_sums<1>(t, out, divide);
    else if (H <= 2) launch_hap_sums<2>(t, out, divide);
    else if (H <= 4) launch_hap_sums<4>(t, out, divide);
    else if (H <= 8) launch_hap_sums<8>(t, out, divide);
    else if (H <= 16) launch_hap_sums<16>(t, out, divide);
    else launch_hap_sums<32>(t, out, divide);
}

int new_values(gbrs_tensor *t) {
    const uint64_t n1 = std::max<uint64_t>(t->st->N, 1);
    GBRS_TRY(t->val.alloc(n1));
    GBRS_TRY(t->elim.alloc(n1));
    return GBRS_OK;
}

}  // namespace

extern "C" {

int gbrs_tensor_create(uint64_t R, uint32_t L, uint32_t H, const uint32_t *const *indptr, const uint32_t *const *indices,
                       const double *const *values, const double *count, int device, gbrs_tensor_t **out) {
    RoctxRange roctx_range("gbrs_tensor_create");
    if (!out) return fail(GBRS_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (H < 1 || H > 32 || L < 1 || R < 1 || R > 0xFFFFFFFFull)
        return fail(GBRS_ERR_INVALID, "The shape must be a tuple of three positive integers (H <= 32, R < 2^32).");
    if (!indptr || !indices) return fail(GBRS_ERR_INVALID, "indptr/indices tables are NULL");
    if (L >= (1u << 27)) return fail(GBRS_ERR_UNSUPPORTED, "the grouped layout holds at most 2^32 - 1 entries of at most 2^27 loci");
    // column offsets of the concatenated CSC arrays (column c = h*L + l), validated on the host
    std::vector<uint64_t> col_ptr((size_t)H * L + 1), hap_off(H + 1);
    uint64_t n = 0;
    for (uint32_t h = 0; h < H; ++h) {
        if (!indptr[h]) return fail(GBRS_ERR_INVALID, "indptr[%u] is NULL", h);
        const uint32_t *p = indptr[h];
        if (p[0] != 0) return fail(GBRS_ERR_INVALID, "indptr[%u][0] != 0", h);
        hap_off[h] = n;
        for (uint32_t l = 0; l < L; ++l) {
            if (p[l + 1] < p[l]) return fail(GBRS_ERR_INVALID, "indptr[%u] is not non-decreasing at %u", h, l);
            col_ptr[(size_t)h * L + l] = n + p[l];
        }
        if (p[L] && !indices[h]) return fail(GBRS_ERR_INVALID, "indices[%u] is NULL", h);
        if (p[L] && values && !values[h]) return fail(GBRS_ERR_INVALID, "values[%u] is NULL", h);
        for (uint32_t k = 0; k < p[L]; ++k)
            if (indices[h][k] >= R) return fail(GBRS_ERR_INVALID, "indices hold row id %u >= num_rows", indices[h][k]);
        n += p[L];
    }
    hap_off[H] = col_ptr[(size_t)H * L] = n;
    if (n >= 0xFFFFFFFFull) return fail(GBRS_ERR_UNSUPPORTED, "the grouped layout holds at most 2^32 - 1 entries of at most 2^27 loci");
    GBRS_TRY(select_device(device));
    std::unique_ptr<gbrs_tensor> t(new gbrs_tensor());
    t->st = std::make_shared<TensorStructure>();
    TensorStructure &st = *t->st;
    st.device = device;
    st.R = R; st.L = L; st.H = H; st.N = n;
    st.hap_off = hap_off;
    GBRS_HIP_CHECK(hipStreamCreateWithFlags(&st.stream, hipStreamDefault));
    GBRS_TRY(st.col_ptr.alloc(col_ptr.size()));
    GBRS_HIP_CHECK(hipMemcpy(st.col_ptr.p, col_ptr.data(), st.col_ptr.bytes(), hipMemcpyHostToDevice));
    GBRS_TRY(st.ent_row.alloc(std::max<uint64_t>(n, 1)));
    GBRS_TRY(new_values(t.get()));
    GBRS_HIP_CHECK(hipMemset(t->elim.p, 0, t->elim.bytes()));
    for (uint32_t h = 0; h < H; ++h) {
        const uint64_t cnt = hap_off[h + 1] - hap_off[h];
        if (cnt == 0) continue;
        GBRS_HIP_CHECK(hipMemcpy(st.ent_row.p + hap_off[h], indices[h], cnt * sizeof(uint32_t), hipMemcpyHostToDevice));
        if (values) GBRS_HIP_CHECK(hipMemcpy(t->val.p + hap_off[h], values[h], cnt * sizeof(double), hipMemcpyHostToDevice));
    }
    if (count) {
        st.has_count = true;
        GBRS_TRY(st.count.alloc(R));
        GBRS_HIP_CHECK(hipMemcpy(st.count.p, count, R * sizeof(double), hipMemcpyHostToDevice));
    }
    GBRS_TRY(st.acc.alloc((size_t)H * L));
    GBRS_TRY(st.nnz.alloc(H));
    GBRS_TRY(st.flag.alloc(1));
    GBRS_TRY(build_row_ptr(st.row_ptr, R, n, st.ent_row.p, st.stream));
    GBRS_TRY(set_groups_impl(st, 0, nullptr, nullptr));
    if (!values) GBRS_TRY(launch_elementwise(t.get(), FORM_RESET, nullptr));
    *out = t.release();
    return GBRS_OK;
}

int gbrs_tensor_set_groups(gbrs_tensor_t *t, int64_t G, const int64_t *group_ptr, const int64_t *members) {
    RoctxRange roctx_range("gbrs_tensor_set_groups");
    if (!t || G < 0 || (G > 0 && (!group_ptr || !members))) return fail(GBRS_ERR_INVALID, "bad argument");
    GBRS_TRY(check_handle(t));
    return set_groups_impl(*t->st, G, group_ptr, members);
}

int gbrs_tensor_reset(gbrs_tensor_t *t) {
    RoctxRange roctx_range("gbrs_tensor_reset");
    GBRS_TRY(check_handle(t));
    return launch_elementwise(t, FORM_RESET, nullptr);
}

int gbrs_tensor_multiply(gbrs_tensor_t *t, int form, const double *m, uint64_t m_len) {
    RoctxRange roctx_range("gbrs_tensor_multiply");
    GBRS_TRY(check_handle(t));
    TensorStructure &st = *t->st;
    uint64_t want = 0;
    switch (form) {
    case FORM_LOCUS: want = st.L; break;
    case FORM_READ: want = st.R; break;
    case FORM_READ_HAP: want = st.R * st.H; break;
    case FORM_HAP_LOCUS: want = (uint64_t)st.H * st.L; break;
    default: return fail(GBRS_ERR_INVALID, "multiply form %d is not one of 1 (locus), 2 (read), 3 (read x haplotype), 4 (haplotype x locus)", form);
    }
    if (!m) return fail(GBRS_ERR_INVALID, "the multiplier is NULL");
    if (m_len != want)
        return fail(GBRS_ERR_INVALID, "the multiplier holds %llu values, form %d needs %llu", (unsigned long long)m_len, form,
                    (unsigned long long)want);
    if (st.mult.n < want) GBRS_TRY(st.mult.alloc(want));
    GBRS_HIP_CHECK(hipMemcpyAsync(st.mult.p, m, want * sizeof(double), hipMemcpyHostToDevice, st.stream));
    return launch_elementwise(t, form, st.mult.p);
}

int gbrs_tensor_multiply_tensor(gbrs_tensor_t *t, const gbrs_tensor_t *other) {
    RoctxRange roctx_range("gbrs_tensor_multiply_tensor");
    GBRS_TRY(check_handle(t));
    if (!other) return fail(GBRS_ERR_INVALID, "the multiplier handle is NULL");
    if (other->st != t->st)
        return fail(GBRS_ERR_UNSUPPORTED, "multiply with a tensor of another structure (only a copy() of the same tensor)");
    return launch_elementwise(t, FORM_TENSOR, other->val.p);      // (other == t squares the values: one read, one write per lane)
}

int gbrs_tensor_normalize(gbrs_tensor_t *t, int axis) {
    RoctxRange roctx_range("gbrs_tensor_normalize");
    GBRS_TRY(check_handle(t));
    if (axis < AX_LOCUS || axis > AX_HAPLOGROUP) return fail(GBRS_ERR_INVALID, "The axis should be 0, 1, 2, 3, or 4.");
    TensorStructure &st = *t->st;
    if (st.N == 0) return GBRS_OK;
    const bool hap_major = axis == AX_HAPLOGROUP;
    GBRS_TRY(ensure_order(st, hap_major));
    GBRS_TRY(clear_flag(st));
    const GroupedOrder &o = hap_major ? st.order_hl : st.order_lh;
#define GBRS_LAUNCH_NORMALIZE(AX)                                                                                      \
    hipLaunchKernelGGL(tensor_normalize_kernel<AX>, dim3(grid_for(st.R)), dim3(256), 0, st.stream, st.R, st.row_ptr.p,  \
                       o.lh.p, o.src.p, st.locus_gene.p, t->val.p, t->elim.p, st.flag.p)
    switch (axis) {
    case AX_LOCUS: GBRS_LAUNCH_NORMALIZE(AX_LOCUS); break;
    case AX_READ: GBRS_LAUNCH_NORMALIZE(AX_READ); break;
    case AX_GROUP: GBRS_LAUNCH_NORMALIZE(AX_GROUP); break;
    case AX_HAPLOGROUP: GBRS_LAUNCH_NORMALIZE(AX_HAPLOGROUP); break;
    default: dispatch_hap_sums(t, nullptr, true); break;
    }
#undef GBRS_LAUNCH_NORMALIZE
    return check_float(st);
}

int gbrs_tensor_sum_reads(gbrs_tensor_t *t, double *out_HxL) {
    RoctxRange roctx_range("gbrs_tensor_sum_reads");
    GBRS_TRY(check_handle(t));
    if (!out_HxL) return fail(GBRS_ERR_INVALID, "out is NULL");
    TensorStructure &st = *t->st;
    GBRS_HIP_CHECK(hipMemsetAsync(st.acc.p, 0, st.acc.bytes(), st.stream));
    if (st.N)
        hipLaunchKernelGGL(tensor_sum_reads_kernel, dim3(grid_for(st.N)), dim3(256), 0, st.stream, st.N, st.H * st.L,
                           st.col_ptr.p, st.ent_row.p, t->val.p, st.has_count ? st.count.p : (const double *)nullptr, st.acc.p);
    GBRS_HIP_CHECK(hipGetLastError());
    GBRS_HIP_CHECK(hipMemcpyAsync(out_HxL, st.acc.p, st.acc.bytes(), hipMemcpyDeviceToHost, st.stream));
    GBRS_HIP_CHECK(hipStreamSynchronize(st.stream));
    return GBRS_OK;
}

int gbrs_tensor_sum_loci(gbrs_tensor_t *t, double *out_RxH) {
    RoctxRange roctx_range("gbrs_tensor_sum_loci");
    GBRS_TRY(check_handle(t));
    if (!out_RxH) return fail(GBRS_ERR_INVALID, "out is NULL");
    TensorStructure &st = *t->st;
    GBRS_TRY(ensure_order(st, false));
    if (!st.rows_out.p) GBRS_TRY(st.rows_out.alloc(st.R * st.H));
    dispatch_hap_sums(t, st.rows_out.p, false);            // (a read without entries stores zeros)
    GBRS_HIP_CHECK(hipGetLastError());
    GBRS_HIP_CHECK(hipMemcpyAsync(out_RxH, st.rows_out.p, st.rows_out.bytes(), hipMemcpyDeviceToHost, st.stream));
    GBRS_HIP_CHECK(hipStreamSynchronize(st.stream));
    return GBRS_OK;
}

int gbrs_tensor_copy(gbrs_tensor_t *t, gbrs_tensor_t **out) {
    RoctxRange roctx_range("gbrs_tensor_copy");
    if (!out) return fail(GBRS_ERR_INVALID, "out is NULL");
    *out = nullptr;
    GBRS_TRY(check_handle(t));
    std::unique_ptr<gbrs_tensor> c(new gbrs_tensor());
    c->st = t->st;
    GBRS_TRY(new_values(c.get()));
    hipStream_t s = t->st->stream;
    GBRS_HIP_CHECK(hipMemcpyAsync(c->val.p, t->val.p, t->val.bytes(), hipMemcpyDeviceToDevice, s));
    GBRS_HIP_CHECK(hipMemcpyAsync(c->elim.p, t->elim.p, t->elim.bytes(), hipMemcpyDeviceToDevice, s));
    GBRS_HIP_CHECK(hipStreamSynchronize(s));
    *out = c.release();
    return GBRS_OK;
}

int gbrs_tensor_values(gbrs_tensor_t *t, uint32_t hap, double *out, uint8_t *live, uint64_t len) {
    GBRS_TRY(check_handle(t));
    TensorStructure &st = *t->st;
    if (hap >= st.H) return fail(GBRS_ERR_INVALID, "haplotype %u out of range", hap);
    const uint64_t first = st.hap_off[hap], cnt = st.hap_off[hap + 1] - first;
    if (len != cnt)
        return fail(GBRS_ERR_INVALID, "haplotype %u holds %llu entries, the buffer %llu", hap, (unsigned long long)cnt,
                    (unsigned long long)len);
    if (cnt == 0) return GBRS_OK;
    if (!out && !live) return fail(GBRS_ERR_INVALID, "out and live are both NULL");
    if (out) GBRS_HIP_CHECK(hipMemcpyAsync(out, t->val.p + first, cnt * sizeof(double), hipMemcpyDeviceToHost, st.stream));
    if (live) GBRS_HIP_CHECK(hipMemcpyAsync(live, t->elim.p + first, cnt, hipMemcpyDeviceToHost, st.stream));
    GBRS_HIP_CHECK(hipStreamSynchronize(st.stream));
    if (live)
        for (uint64_t k = 0; k < cnt; ++k) live[k] = !live[k];
    return GBRS_OK;
}

int gbrs_tensor_set_values(gbrs_tensor_t *t, uint32_t hap, const double *v, uint64_t len) {
    GBRS_TRY(check_handle(t));
    TensorStructure &st = *t->st;
    if (hap >= st.H) return fail(GBRS_ERR_INVALID, "haplotype %u out of range", hap);
    const uint64_t first = st.hap_off[hap], cnt = st.hap_off[hap + 1] - first;
    if (len != cnt)
        return fail(GBRS_ERR_INVALID, "haplotype %u holds %llu entries, the buffer %llu", hap, (unsigned long long)cnt,
                    (unsigned long long)len);
    if (cnt == 0) return GBRS_OK;
    if (!v) return fail(GBRS_ERR_INVALID, "the values are NULL");
    GBRS_HIP_CHECK(hipMemcpyAsync(t->val.p + first, v, cnt * sizeof(double), hipMemcpyHostToDevice, st.stream));
    hipLaunchKernelGGL(tensor_clear_eliminated_kernel, dim3(grid_for(cnt)), dim3(256), 0, st.stream, first, first + cnt,
                       t->elim.p, t->val.p);
    GBRS_HIP_CHECK(hipGetLastError());
    GBRS_HIP_CHECK(hipStreamSynchronize(st.stream));
    return GBRS_OK;
}

int gbrs_tensor_nnz(gbrs_tensor_t *t, uint64_t *per_hap) {
    GBRS_TRY(check_handle(t));
    if (!per_hap) return fail(GBRS_ERR_INVALID, "per_hap is NULL");
    TensorStructure &st = *t->st;
    GBRS_HIP_CHECK(hipMemsetAsync(st.nnz.p, 0, st.nnz.bytes(), st.stream));
    for (uint32_t h = 0; h < st.H; ++h) {
        const uint64_t first = st.hap_off[h], end = st.hap_off[h + 1];
        if (end > first)
            hipLaunchKernelGGL(tensor_count_live_kernel, dim3(grid_for(end - first)), dim3(256), 0, st.stream, first, end,
                               t->elim.p, st.nnz.p + h);
    }
    GBRS_HIP_CHECK(hipGetLastError());
    std::vector<unsigned long long> host(st.H);
    GBRS_HIP_CHECK(hipMemcpyAsync(host.data(), st.nnz.p, st.nnz.bytes(), hipMemcpyDeviceToHost, st.stream));
    GBRS_HIP_CHECK(hipStreamSynchronize(st.stream));
    for (uint32_t h = 0; h < st.H; ++h) per_hap[h] = host[h];
    return GBRS_OK;
}

int gbrs_tensor_destroy(gbrs_tensor_t *t) {
    if (!t) return GBRS_OK;
    if (t->st) (void)select_device(t->st->device);
    delete t;
    return GBRS_OK;
}

}  // extern "C"
