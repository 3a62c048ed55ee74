// rocPRIM scans and radix sorts with one reusable temporary buffer, shared by the translation units that
// build layouts on the device (em_layout.hip, bam.hip, matops.hip).
#pragma once
#include "common.h"

#include <rocprim/rocprim.hpp>

namespace gbrs {

// ---- rocPRIM wrappers with one reusable temporary buffer ------------------------------------
struct Scratch {
    DevBuf<unsigned char> buf;
    int reserve(size_t bytes) {
        if (bytes <= buf.n) return GBRS_OK;
        return buf.alloc(bytes + (bytes >> 2) + 256);
    }
};

#define GBRS_PRIM(expr) GBRS_HIP_CHECK(expr)

template <typename T>
int exclusive_scan(Scratch &sc, const T *in, T *out, size_t n, hipStream_t s) {
    if (n == 0) return GBRS_OK;
    size_t bytes = 0;
    GBRS_PRIM(rocprim::exclusive_scan(nullptr, bytes, in, out, T(0), n, rocprim::plus<T>(), s));
    GBRS_TRY(sc.reserve(bytes));
    GBRS_PRIM(rocprim::exclusive_scan(sc.buf.p, bytes, in, out, T(0), n, rocprim::plus<T>(), s));
    return GBRS_OK;
}

template <typename T>
int inclusive_scan(Scratch &sc, const T *in, T *out, size_t n, hipStream_t s) {
    if (n == 0) return GBRS_OK;
    size_t bytes = 0;
    GBRS_PRIM(rocprim::inclusive_scan(nullptr, bytes, in, out, n, rocprim::plus<T>(), s));
    GBRS_TRY(sc.reserve(bytes));
    GBRS_PRIM(rocprim::inclusive_scan(sc.buf.p, bytes, in, out, n, rocprim::plus<T>(), s));
    return GBRS_OK;
}

inline int sort_keys64(Scratch &sc, const uint64_t *in, uint64_t *out, size_t n, unsigned end_bit, hipStream_t s) {
    if (n == 0) return GBRS_OK;
    size_t bytes = 0;
    GBRS_PRIM(rocprim::radix_sort_keys(nullptr, bytes, in, out, n, 0u, end_bit, s));
    GBRS_TRY(sc.reserve(bytes));
    GBRS_PRIM(rocprim::radix_sort_keys(sc.buf.p, bytes, in, out, n, 0u, end_bit, s));
    return GBRS_OK;
}

template <typename K>
int sort_pairs(Scratch &sc, const K *kin, K *kout, const uint32_t *vin, uint32_t *vout, size_t n,
               unsigned end_bit, hipStream_t s) {
    if (n == 0) return GBRS_OK;
    size_t bytes = 0;
    GBRS_PRIM(rocprim::radix_sort_pairs(nullptr, bytes, kin, kout, vin, vout, n, 0u, end_bit, s));
    GBRS_TRY(sc.reserve(bytes));
    GBRS_PRIM(rocprim::radix_sort_pairs(sc.buf.p, bytes, kin, kout, vin, vout, n, 0u, end_bit, s));
    return GBRS_OK;
}

// stable sort on the key bits [begin_bit, end_bit) only
template <typename K>
int sort_pairs_bits(Scratch &sc, const K *kin, K *kout, const uint32_t *vin, uint32_t *vout, size_t n,
                    unsigned begin_bit, unsigned end_bit, hipStream_t s) {
    if (n == 0) return GBRS_OK;
    size_t bytes = 0;
    GBRS_PRIM(rocprim::radix_sort_pairs(nullptr, bytes, kin, kout, vin, vout, n, begin_bit, end_bit, s));
    GBRS_TRY(sc.reserve(bytes));
    GBRS_PRIM(rocprim::radix_sort_pairs(sc.buf.p, bytes, kin, kout, vin, vout, n, begin_bit, end_bit, s));
    return GBRS_OK;
}

// distinct values of a sorted array, in order; *count_out (device) receives how many
inline int unique_keys64(Scratch &sc, const uint64_t *in, uint64_t *out, uint64_t *count_out, size_t n, hipStream_t s) {
    if (n == 0) return GBRS_OK;
    size_t bytes = 0;
    GBRS_PRIM(rocprim::unique(nullptr, bytes, in, out, count_out, n, rocprim::equal_to<uint64_t>(), s));
    GBRS_TRY(sc.reserve(bytes));
    GBRS_PRIM(rocprim::unique(sc.buf.p, bytes, in, out, count_out, n, rocprim::equal_to<uint64_t>(), s));
    return GBRS_OK;
}

// segmented sum over runs of equal keys (keys sorted): distinct keys, their uint32 sums, *count_out (device) = runs.
// Integer addition: the result does not depend on how the runs are cut into blocks.
template <typename ValueIt>
int sum_by_key64(Scratch &sc, const uint64_t *kin, ValueIt vin, uint64_t *kout, uint32_t *vout, uint64_t *count_out,
                 size_t n, hipStream_t s) {
    if (n == 0) return GBRS_OK;
    size_t bytes = 0;
    GBRS_PRIM(rocprim::reduce_by_key(nullptr, bytes, kin, vin, n, kout, vout, count_out, rocprim::plus<uint32_t>(),
                                     rocprim::equal_to<uint64_t>(), s));
    GBRS_TRY(sc.reserve(bytes));
    GBRS_PRIM(rocprim::reduce_by_key(sc.buf.p, bytes, kin, vin, n, kout, vout, count_out, rocprim::plus<uint32_t>(),
                                     rocprim::equal_to<uint64_t>(), s));
    return GBRS_OK;
}

template <typename T>
int fetch_last_plus(const T *scan_out, const T *in, size_t n, T &total, hipStream_t s) {
    // total of an exclusive scan = last output + last input
    T a = 0, b = 0;
    if (n) {
        GBRS_HIP_CHECK(hipMemcpyAsync(&a, scan_out + n - 1, sizeof(T), hipMemcpyDeviceToHost, s));
        GBRS_HIP_CHECK(hipMemcpyAsync(&b, in + n - 1, sizeof(T), hipMemcpyDeviceToHost, s));
        GBRS_HIP_CHECK(hipStreamSynchronize(s));
    }
    total = a + b;
    return GBRS_OK;
}

inline unsigned bits_for(uint64_t max_value) {
    unsigned b = 1;
    while (b < 64 && (max_value >> b)) ++b;
    return b;
}

inline unsigned grid_for(uint64_t n, unsigned block = 256) { return (unsigned)((n + block - 1) / block); }

}  // namespace gbrs
