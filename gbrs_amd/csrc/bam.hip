// Device stages of `gbrs bam2emase`: rank the read names, build the per-haplotype CSC incidence matrices; and of
// `gbrs bam2ec` (gbrs_ecset_*, at the end of the file): the same two stages without the names, then the equivalence
// classes of the file from the arrays where they lie, merged into the classes of the files before it; for a
// paired-end sample (gbrs_ecset_add_bam_pair) both ends are converted, their sorted names compared and the entries
// both ends have kept, all on the device, before the class build.
// rocPRIM provides the radix sorts and scans (prim.h); the kernels around them are written here.
//
// Names.  The host pass (bamio.hip) hands over C candidate names (every record's name, except that a record
// named like its predecessor reuses the predecessor's candidate).  Name c is packed into W = ceil(longest / 8)
// big-endian 64-bit words, zero padded, stored as W planes of C words: planes[w * C + c].  Zero sorts before every
// byte a name may hold, so comparing the word tuples is comparing the names bytewise with a prefix first -
// the order of Python's sorted() on ASCII names.  A stable least-significant-word-first radix sort of a
// permutation ranks them: one pass per plane, last plane first, each pass gathering the plane through the
// current permutation (coalesced write, random 8-byte reads).  One AND/OR reduction per plane finds the bits
// that differ between any two candidates; a plane with none is skipped (Illumina names share a 20-30 byte
// prefix), and the others sort only the bit range that differs.  Adjacent sorted names that differ open a new
// read id (flag + inclusive scan); rank[candidate] = read id.
//
// Matrix.  Every kept record (candidate, refID) becomes the 64-bit key (haplotype * L + locus) << rbits | read id
// through the per-reference table; a sort, a neighbour compare and a scan leave each (haplotype, locus, read)
// once, in CSC order: the low words are `indices`, and the positions where the column changes are `indptr`.
#include "bamio.h"
#include "em_layout.h"
#include "prim.h"

#include <algorithm>

namespace gbrs {
namespace {

constexpr int MAX_PLANES = 32;                 // l_read_name is one byte: names hold at most 254 bytes
struct PlaneList { int n; int w[MAX_PLANES]; };

__device__ __forceinline__ uint64_t wave_and(uint64_t v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v &= __shfl_xor(v, off, WAVE);
    return v;
}
__device__ __forceinline__ uint64_t wave_or(uint64_t v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v |= __shfl_xor(v, off, WAVE);
    return v;
}

// one thread per (candidate, word): the candidate index runs fastest, so a wavefront writes 512 contiguous bytes
// of one plane and reads 64 neighbouring names
__global__ void __launch_bounds__(256)
pack_names_kernel(uint64_t C, uint32_t W, const unsigned char *__restrict__ bytes, uint64_t n_bytes,
                  const uint64_t *__restrict__ off, uint64_t *__restrict__ planes) {
    const uint64_t total = C * W;
    for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t w = t / C, c = t - w * C;
        const uint64_t b0 = off[c], b1 = min(off[c + 1], n_bytes);        // (offsets come from the host: clamp anyway)
        uint64_t word = 0;
        const uint64_t at = b0 + w * 8;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const uint64_t p = at + k;
            const uint64_t byte = p < b1 ? bytes[p] : 0;
            word |= byte << (56 - 8 * k);
        }
        planes[t] = word;
    }
}

// blockIdx.y = plane; per wavefront one atomic pair
__global__ void __launch_bounds__(256)
plane_and_or_kernel(uint64_t C, const uint64_t *__restrict__ planes, unsigned long long *__restrict__ and_out,
                    unsigned long long *__restrict__ or_out) {
    const uint64_t *pl = planes + (uint64_t)blockIdx.y * C;
    uint64_t a = ~0ull, o = 0;
    for (uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; c < C; c += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t v = pl[c];
        a &= v;
        o |= v;
    }
    a = wave_and(a);
    o = wave_or(o);
    if ((threadIdx.x & 63) == 0) {
        atomicAnd(&and_out[blockIdx.y], (unsigned long long)a);
        atomicOr(&or_out[blockIdx.y], (unsigned long long)o);
    }
}

__global__ void __launch_bounds__(256)
iota_kernel(uint64_t n, uint32_t *__restrict__ out) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x)
        out[i] = (uint32_t)i;
}

// perm holds a permutation of 0..n-1 (iota pushed through stable sorts), so plane[perm[i]] is in range
__global__ void __launch_bounds__(256)
gather_plane_kernel(uint64_t n, const uint64_t *__restrict__ plane, const uint32_t *__restrict__ perm,
                    uint64_t *__restrict__ keys) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x)
        keys[i] = plane[perm[i]];
}

// flag[i] = 1 where sorted name i differs from sorted name i - 1 (only the planes that vary are compared)
__global__ void __launch_bounds__(256)
name_boundary_kernel(uint64_t C, PlaneList act, const uint64_t *__restrict__ planes, const uint32_t *__restrict__ perm,
                     uint32_t *__restrict__ flag) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < C; i += (uint64_t)gridDim.x * blockDim.x) {
        uint32_t f = 0;
        if (i > 0) {
            const uint32_t a = perm[i], b = perm[i - 1];
            for (int k = 0; k < act.n; ++k) {
                const uint64_t *pl = planes + (uint64_t)act.w[k] * C;
                f |= pl[a] != pl[b];
            }
        }
        flag[i] = f;
    }
}

__global__ void __launch_bounds__(256)
scatter_rank_kernel(uint64_t C, const uint32_t *__restrict__ perm, const uint32_t *__restrict__ id,
                    uint32_t *__restrict__ rank) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < C; i += (uint64_t)gridDim.x * blockDim.x)
        rank[perm[i]] = id[i];
}

// one thread per (sorted position, word), the word running fastest: the first candidate of every distinct name
// writes its bytes to rname[id][...]; a wavefront writes neighbouring 8-byte pieces
__global__ void __launch_bounds__(256)
gather_rname_kernel(uint64_t C, uint32_t W, uint32_t width, uint64_t R, const uint64_t *__restrict__ planes,
                    const uint32_t *__restrict__ perm, const uint32_t *__restrict__ id, const uint32_t *__restrict__ flag,
                    unsigned char *__restrict__ rname) {
    const uint64_t total = C * W;
    for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t i = t / W;
        const uint32_t w = (uint32_t)(t - i * W);
        if (i > 0 && !flag[i]) continue;
        const uint64_t r = id[i];
        if (r >= R) continue;                       // cannot happen (id is a scan of the flags); keeps the store in range
        const uint64_t word = planes[(uint64_t)w * C + perm[i]];
        unsigned char *dst = rname + r * width + (uint64_t)w * 8;
        const uint32_t nb = min(8u, width - w * 8);
        for (uint32_t k = 0; k < nb; ++k) dst[k] = (unsigned char)(word >> (56 - 8 * k));
    }
}

struct Rec { uint32_t cand; int32_t refid; };
constexpr uint64_t REF_UNUSABLE = ~0ull;

// key = (haplotype * L + locus) << rbits | read id.  A record whose candidate or reference is out of range, or
// whose reference is unusable, is reported (the smallest such record index) and gets key 0.
__global__ void __launch_bounds__(256)
record_keys_kernel(uint64_t N, const Rec *__restrict__ recs, uint64_t C, uint64_t n_ref, const uint64_t *__restrict__ refmap,
                   const uint32_t *__restrict__ rank, uint32_t L, unsigned rbits, uint64_t *__restrict__ keys,
                   unsigned long long *first_bad) {
    for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < N; j += (uint64_t)gridDim.x * blockDim.x) {
        const Rec r = recs[j];
        uint64_t key = 0;
        bool bad = r.cand >= C || r.refid < 0 || (uint64_t)r.refid >= n_ref;
        if (!bad) {
            const uint64_t m = refmap[r.refid];
            bad = m == REF_UNUSABLE;
            if (!bad) key = (((m >> 32) * L + (m & 0xFFFFFFFFu)) << rbits) | rank[r.cand];
        }
        if (bad) atomicMin(first_bad, (unsigned long long)j);
        keys[j] = key;
    }
}

__global__ void __launch_bounds__(256)
unique_flag_kernel(uint64_t N, const uint64_t *__restrict__ keys, uint32_t *__restrict__ flag) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += (uint64_t)gridDim.x * blockDim.x)
        flag[i] = (i == 0 || keys[i] != keys[i - 1]) ? 1u : 0u;
}

// pos = exclusive scan of flag.  Every first occurrence writes its read id; where the column changes, the
// columns passed over (empty ones included) start here.  Columns are < ncols because record_keys_kernel
// rejected everything else and the table's entries were range-checked when it was set.
__global__ void __launch_bounds__(256)
compact_kernel(uint64_t N, const uint64_t *__restrict__ keys, const uint32_t *__restrict__ flag,
               const uint32_t *__restrict__ pos, unsigned rbits, uint64_t ncols, uint32_t *__restrict__ out_idx,
               uint64_t *__restrict__ col_ptr) {
    const uint64_t rmask = rbits >= 64 ? ~0ull : ((1ull << rbits) - 1);
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t key = keys[i];
        const uint64_t col = min(key >> rbits, ncols - 1);
        const uint32_t p = pos[i];
        if (flag[i]) {
            out_idx[p] = (uint32_t)(key & rmask);
            const uint64_t first = i == 0 ? 0 : min(keys[i - 1] >> rbits, ncols - 1) + 1;
            for (uint64_t c = first; c <= col; ++c) col_ptr[c] = p;
        }
        if (i == N - 1) {
            const uint64_t total = (uint64_t)p + flag[i];
            for (uint64_t c = col + 1; c <= ncols; ++c) col_ptr[c] = total;
        }
    }
}

inline unsigned capped_grid(uint64_t n) { return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>((n + 255) / 256, 4096)); }

struct DevResult {
    int device = 0;
    DevBuf<uint32_t> idx;
    DevBuf<unsigned char> rname;
};
void free_result(void *p) {
    DevResult *r = static_cast<DevResult *>(p);
    (void)hipSetDevice(r->device);
    delete r;
}

double seconds_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
}

// candidates -> rank[candidate] (device), R and, when `rname` is given, the sorted distinct names (device).
// rname == nullptr (gbrs_ecset_add_bam): the pass ends with scatter_rank_kernel - no name array is allocated,
// gathered or copied
int rank_names(gbrs_bam *b, Scratch &sc, DevBuf<uint32_t> &rank, DevBuf<unsigned char> *rname, hipStream_t s) {
    const uint64_t C = b->cand_off.size() - 1;
    const uint32_t width = std::max<uint32_t>(b->max_name, 1), W = (width + 7) / 8;
    if (W > MAX_PLANES) return fail(GBRS_ERR_INVALID, "a read name of %u bytes (the format allows 254)", b->max_name);
    DevBuf<unsigned char> bytes;
    DevBuf<uint64_t> off, planes, kin, kout;
    DevBuf<unsigned long long> andor;
    DevBuf<uint32_t> perm, perm2, flag, id;
    const uint64_t n_bytes = b->cand_bytes.size();
    GBRS_TRY(bytes.alloc(std::max<uint64_t>(n_bytes, 1)));
    GBRS_TRY(off.alloc(C + 1));
    GBRS_TRY(planes.alloc(C * W));
    GBRS_TRY(andor.alloc(2 * MAX_PLANES));
    if (n_bytes) GBRS_HIP_CHECK(hipMemcpyAsync(bytes.p, b->cand_bytes.data(), n_bytes, hipMemcpyHostToDevice, s));
    GBRS_HIP_CHECK(hipMemcpyAsync(off.p, b->cand_off.data(), (C + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(pack_names_kernel, dim3(capped_grid(C * W)), dim3(256), 0, s, C, W, bytes.p, n_bytes, off.p, planes.p);
    GBRS_HIP_CHECK(hipGetLastError());
    unsigned long long h_andor[2 * MAX_PLANES];
    for (int w = 0; w < MAX_PLANES; ++w) { h_andor[w] = ~0ull; h_andor[MAX_PLANES + w] = 0; }
    GBRS_HIP_CHECK(hipMemcpyAsync(andor.p, h_andor, sizeof(h_andor), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(plane_and_or_kernel, dim3(std::min(capped_grid(C), 1024u), W), dim3(256), 0, s, C, planes.p, andor.p,
                       andor.p + MAX_PLANES);
    GBRS_HIP_CHECK(hipGetLastError());
    GBRS_HIP_CHECK(hipMemcpyAsync(h_andor, andor.p, sizeof(h_andor), hipMemcpyDeviceToHost, s));
    GBRS_HIP_CHECK(hipStreamSynchronize(s));
    bytes.release();
    off.release();

    GBRS_TRY(perm.alloc(C));
    GBRS_TRY(perm2.alloc(C));
    GBRS_TRY(kin.alloc(C));
    GBRS_TRY(kout.alloc(C));
    hipLaunchKernelGGL(iota_kernel, dim3(capped_grid(C)), dim3(256), 0, s, C, perm.p);
    GBRS_HIP_CHECK(hipGetLastError());
    PlaneList act;
    act.n = 0;
    for (int w = (int)W - 1; w >= 0; --w) {
        const uint64_t diff = h_andor[w] ^ h_andor[MAX_PLANES + w];      // bits on which two candidates differ
        if (!diff) continue;
        act.w[act.n++] = w;
        const unsigned begin_bit = (unsigned)__builtin_ctzll(diff), end_bit = 64u - (unsigned)__builtin_clzll(diff);
        hipLaunchKernelGGL(gather_plane_kernel, dim3(capped_grid(C)), dim3(256), 0, s, C, planes.p + (uint64_t)w * C, perm.p, kin.p);
        GBRS_HIP_CHECK(hipGetLastError());
        GBRS_TRY(sort_pairs_bits(sc, kin.p, kout.p, perm.p, perm2.p, C, begin_bit, end_bit, s));
        perm.swap(perm2);
    }
    kin.release();
    kout.release();
    perm2.release();
    GBRS_TRY(flag.alloc(C));
    GBRS_TRY(id.alloc(C));
    hipLaunchKernelGGL(name_boundary_kernel, dim3(capped_grid(C)), dim3(256), 0, s, C, act, planes.p, perm.p, flag.p);
    GBRS_HIP_CHECK(hipGetLastError());
    GBRS_TRY(inclusive_scan(sc, flag.p, id.p, C, s));
    uint32_t last = 0;
    GBRS_HIP_CHECK(hipMemcpyAsync(&last, id.p + C - 1, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    GBRS_HIP_CHECK(hipStreamSynchronize(s));
    const uint64_t R = (uint64_t)last + 1;
    GBRS_TRY(rank.alloc(C));
    hipLaunchKernelGGL(scatter_rank_kernel, dim3(capped_grid(C)), dim3(256), 0, s, C, perm.p, id.p, rank.p);
    GBRS_HIP_CHECK(hipGetLastError());
    if (rname) {
        GBRS_TRY(rname->alloc(R * width));
        GBRS_HIP_CHECK(hipMemsetAsync(rname->p, 0, R * width, s));
        hipLaunchKernelGGL(gather_rname_kernel, dim3(capped_grid(C * W)), dim3(256), 0, s, C, W, width, R, planes.p, perm.p, id.p,
                           flag.p, rname->p);
        GBRS_HIP_CHECK(hipGetLastError());
    }
    GBRS_HIP_CHECK(hipStreamSynchronize(s));
    b->num_reads = R;
    b->name_width = width;
    return GBRS_OK;
}

int report_bad_record(gbrs_bam *b, uint64_t j) {
    const gbrs_bam::Rec r = b->recs[j];
    std::string read = "?";
    if ((uint64_t)r.cand + 1 < b->cand_off.size())
        read.assign((const char *)b->cand_bytes.data() + b->cand_off[r.cand], (size_t)(b->cand_off[r.cand + 1] - b->cand_off[r.cand]));
    if (r.refid < 0 || (size_t)r.refid >= b->ref_names.size())
        return fail(GBRS_ERR_INVALID, "%s: read '%s' has a record without a reference sequence (refID %d) whose flag is neither 4 nor 8",
                    b->path.c_str(), read.c_str(), r.refid);
    const char *ref = b->ref_names[r.refid].c_str();
    switch (b->ref_locus[r.refid]) {
    case BAM_REF_NOT_TWO_PARTS:
        return fail(GBRS_ERR_INVALID, "%s: reference sequence '%s' (read '%s') does not split into exactly (locus, haplotype) at the delimiter",
                    b->path.c_str(), ref, read.c_str());
    case BAM_REF_UNKNOWN_HAPLOTYPE:
        return fail(GBRS_ERR_INVALID, "%s: reference sequence '%s' (read '%s') names a haplotype that was not given", b->path.c_str(), ref, read.c_str());
    default:
        return fail(GBRS_ERR_INVALID, "%s: reference sequence '%s' (read '%s') names a locus that is not in the locus id file", b->path.c_str(), ref, read.c_str());
    }
}

// idx / col_ptr: the entries' read ids in CSC order and the H * L + 1 column offsets, both on the device (left
// unallocated when no record is kept); b->col_ptr receives the offsets on the host
int build_matrix(gbrs_bam *b, Scratch &sc, const DevBuf<uint32_t> &rank, DevBuf<uint32_t> &idx, DevBuf<uint64_t> &col_ptr,
                 hipStream_t s) {
    const uint64_t N = b->recs.size(), C = b->cand_off.size() - 1, R = b->num_reads, n_ref = b->ref_names.size();
    const uint64_t ncols = (uint64_t)b->num_haps * b->num_loci;
    const unsigned rbits = bits_for(R - 1), cbits = bits_for(ncols - 1);
    if (rbits + cbits > 64)
        return fail(GBRS_ERR_UNSUPPORTED, "%u haplotypes x %u loci x %llu reads do not fit a 64-bit key", b->num_haps, b->num_loci, (unsigned long long)R);
    if (N > 0xFFFFFFFFull) return fail(GBRS_ERR_UNSUPPORTED, "more than 2^32 - 1 alignment records to keep");
    b->col_ptr.assign(ncols + 1, 0);
    if (N == 0) return GBRS_OK;
    DevBuf<Rec> recs;
    DevBuf<uint64_t> refmap, kin, kout;
    DevBuf<unsigned long long> first_bad;
    DevBuf<uint32_t> flag, pos;
    std::vector<uint64_t> h_map(std::max<uint64_t>(n_ref, 1), REF_UNUSABLE);
    for (uint64_t k = 0; k < n_ref; ++k)
        if (b->ref_hap[k] != BAM_REF_UNUSABLE) h_map[k] = ((uint64_t)b->ref_hap[k] << 32) | b->ref_locus[k];
    GBRS_TRY(recs.alloc(N));
    GBRS_TRY(refmap.alloc(h_map.size()));
    GBRS_TRY(kin.alloc(N));
    GBRS_TRY(kout.alloc(N));
    GBRS_TRY(first_bad.alloc(1));
    static_assert(sizeof(Rec) == sizeof(gbrs_bam::Rec), "record layout");
    GBRS_HIP_CHECK(hipMemcpyAsync(recs.p, b->recs.data(), N * sizeof(Rec), hipMemcpyHostToDevice, s));
    GBRS_HIP_CHECK(hipMemcpyAsync(refmap.p, h_map.data(), h_map.size() * sizeof(uint64_t), hipMemcpyHostToDevice, s));
    GBRS_HIP_CHECK(hipMemsetAsync(first_bad.p, 0xFF, sizeof(unsigned long long), s));
    hipLaunchKernelGGL(record_keys_kernel, dim3(capped_grid(N)), dim3(256), 0, s, N, recs.p, C, n_ref, refmap.p, rank.p, b->num_loci,
                       rbits, kin.p, first_bad.p);
    GBRS_HIP_CHECK(hipGetLastError());
    unsigned long long bad = 0;
    GBRS_HIP_CHECK(hipMemcpyAsync(&bad, first_bad.p, sizeof(bad), hipMemcpyDeviceToHost, s));
    GBRS_HIP_CHECK(hipStreamSynchronize(s));
    if (bad != ~0ull) return report_bad_record(b, std::min<uint64_t>(bad, N - 1));
    recs.release();
    GBRS_TRY(sort_keys64(sc, kin.p, kout.p, N, rbits + cbits, s));
    GBRS_TRY(flag.alloc(N));
    GBRS_TRY(pos.alloc(N));
    hipLaunchKernelGGL(unique_flag_kernel, dim3(capped_grid(N)), dim3(256), 0, s, N, kout.p, flag.p);
    GBRS_HIP_CHECK(hipGetLastError());
    GBRS_TRY(exclusive_scan(sc, flag.p, pos.p, N, s));
    uint32_t n_unique = 0;
    GBRS_TRY(fetch_last_plus(pos.p, flag.p, N, n_unique, s));
    GBRS_TRY(idx.alloc(n_unique));
    GBRS_TRY(col_ptr.alloc(ncols + 1));
    hipLaunchKernelGGL(compact_kernel, dim3(capped_grid(N)), dim3(256), 0, s, N, kout.p, flag.p, pos.p, rbits, ncols, idx.p, col_ptr.p);
    GBRS_HIP_CHECK(hipGetLastError());
    GBRS_HIP_CHECK(hipMemcpyAsync(b->col_ptr.data(), col_ptr.p, (ncols + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    GBRS_HIP_CHECK(hipStreamSynchronize(s));
    if (b->col_ptr[0] != 0 || b->col_ptr[ncols] != n_unique) return fail(GBRS_ERR_HIP, "internal error: column pointers do not span the entries");
    return GBRS_OK;
}

// ---- gbrs_ecset: equivalence classes of several BAM files, merged on the device ---------------------------------
// The set and a file's classes are both class matrices in CSC form (column c = h * L + l, class ids ascending inside
// a column).  Stacking the file's classes below the set's - their ids raised by the set's class count - needs no
// sort: every row of the addend comes after every row of the set, so column c of the stack is the set's column c
// followed by the addend's.  out_ptr = a_ptr + b_ptr gives the columns' places.
__global__ void __launch_bounds__(256)
ecset_merge_ptr_kernel(uint64_t n_ptr, const uint64_t *__restrict__ a_ptr, const uint64_t *__restrict__ b_ptr,
                       uint64_t *__restrict__ out_ptr) {
    for (uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; c < n_ptr; c += (uint64_t)gridDim.x * blockDim.x)
        out_ptr[c] = a_ptr[c] + b_ptr[c];
}

// One operand's entries to their places in the stack: entry k of column c moves up by the entries the OTHER operand
// has before it - for the set (after = 0) the addend's columns before c, other_ptr[c]; for the addend (after = 1) the
// set's columns up to and including c, other_ptr[c + 1].  A wavefront's entries are consecutive in every pass of the
// loop (the stride is a multiple of 256), which is what entry_column needs; dst < n_out holds by construction
// (k - own_ptr[c] < own_ptr[c + 1] - own_ptr[c]) and is checked because the offsets are read from memory.
__global__ void __launch_bounds__(256)
ecset_merge_copy_kernel(uint64_t n, uint32_t ncols, const uint64_t *__restrict__ own_ptr, const uint64_t *__restrict__ other_ptr,
                        uint32_t after, const uint32_t *__restrict__ idx, uint32_t id_offset, uint64_t n_out,
                        uint32_t *__restrict__ out) {
    for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t c = entry_column(own_ptr, ncols, k, n);
        const uint64_t dst = k + other_ptr[c + after];
        if (dst < n_out) out[dst] = idx[k] + id_offset;
    }
}

// ---- gbrs_ecset_add_bam_pair: the two ends of a paired-end sample ------------------------------------------------
// Both ends' sorted distinct names lie on the device as R x width bytes, zero padded.  One thread per (sorted
// position, 8-byte piece), the piece running fastest, so a wavefront reads neighbouring bytes of both arrays; a
// piece is compared as the big-endian word pack_names_kernel would make of it, each array padded with zeros to the
// wider one's width.  first_diff keeps the smallest position whose names differ (the first differing lane of a
// wavefront holds the wavefront's smallest, so one atomic per wavefront and pass); every load is inside R x width.
__global__ void __launch_bounds__(256)
pair_names_differ_kernel(uint64_t R, uint32_t W, const unsigned char *__restrict__ a, uint32_t width_a,
                         const unsigned char *__restrict__ b, uint32_t width_b, unsigned long long *first_diff) {
    const uint64_t total = R * W;
    for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t i = t / W;
        const uint32_t at = (uint32_t)(t - i * W) * 8;
        const unsigned char *na = a + i * width_a, *nb = b + i * width_b;
        uint64_t wa = 0, wb = 0;
#pragma unroll
        for (uint32_t k = 0; k < 8; ++k) {
            const uint32_t p = at + k;
            wa |= (uint64_t)(p < width_a ? na[p] : 0) << (56 - 8 * k);
            wb |= (uint64_t)(p < width_b ? nb[p] : 0) << (56 - 8 * k);
        }
        const bool differ = wa != wb;
        const uint64_t any = __ballot(differ);
        if (differ && (threadIdx.x & 63) == (unsigned)__builtin_ctzll(any)) atomicMin(first_diff, (unsigned long long)i);
    }
}

// flag[k] = entry k of the first end (column c, read r) is an entry of the second end too: bisection for r inside
// the second end's column c, whose read ids ascend.  One lane per entry; the column is found once per wavefront
// (entry_column: the wavefront's entries are consecutive in every pass, the stride being a multiple of 256).
// flag[n] = 0 closes the exclusive scan, so that pos[n] is the number of common entries.  n >= 1.
__global__ void __launch_bounds__(256)
pair_common_flag_kernel(uint64_t n, uint32_t ncols, const uint64_t *__restrict__ a_ptr, const uint32_t *__restrict__ a_idx,
                        const uint64_t *__restrict__ b_ptr, const uint32_t *__restrict__ b_idx, uint64_t n_b,
                        uint32_t *__restrict__ flag) {
    for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k <= n; k += (uint64_t)gridDim.x * blockDim.x) {
        const bool live = k < n;
        const uint32_t c = entry_column(a_ptr, ncols, live ? k : n - 1, n);
        uint32_t f = 0;
        if (live) {
            const uint32_t r = a_idx[k];
            uint64_t lo = min(b_ptr[c], n_b), hi = min(b_ptr[c + 1], n_b);     // first j in [lo, hi) with b_idx[j] >= r
            const uint64_t end = hi;
            while (lo < hi) {
                const uint64_t mid = lo + ((hi - lo) >> 1);
                if (b_idx[mid] < r) lo = mid + 1; else hi = mid;
            }
            f = (lo < end && b_idx[lo] == r) ? 1u : 0u;
        }
        flag[k] = f;
    }
}

// pos = exclusive scan of flag over n + 1 entries: the common entries to their places
__global__ void __launch_bounds__(256)
pair_common_compact_kernel(uint64_t n, const uint32_t *__restrict__ a_idx, const uint32_t *__restrict__ flag,
                           const uint32_t *__restrict__ pos, uint64_t n_out, uint32_t *__restrict__ out) {
    for (uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t p = pos[k];
        if (flag[k] && p < n_out) out[p] = a_idx[k];
    }
}

// column c of the common structure starts after the common entries before the first end's column c: pos[a_ptr[c]],
// whichever columns were emptied (a_ptr[ncols] = n, pos[n] = the total)
__global__ void __launch_bounds__(256)
pair_common_ptr_kernel(uint64_t n_ptr, const uint64_t *__restrict__ a_ptr, const uint32_t *__restrict__ pos, uint64_t n,
                       uint64_t *__restrict__ out_ptr) {
    for (uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; c < n_ptr; c += (uint64_t)gridDim.x * blockDim.x)
        out_ptr[c] = pos[min(a_ptr[c], n)];
}

// one end of a pair, converted: what stays on the device until the pair has been added
struct PairEnd {
    uint64_t R = 0;
    uint32_t width = 1;
    DevBuf<unsigned char> rname;                 // R x width, sorted
    DevBuf<uint32_t> idx;                        // unallocated when no record is kept
    DevBuf<uint64_t> col_ptr;
};

// rank_names + build_matrix of a collected file; the conversion's temporaries are gone when this returns
int convert_end(gbrs_bam *b, PairEnd &end, double *rank_seconds, double *build_seconds, hipStream_t s) {
    Scratch sc;
    DevBuf<uint32_t> rank;
    auto t0 = std::chrono::steady_clock::now();
    int rc = rank_names(b, sc, rank, &end.rname, s);
    *rank_seconds += seconds_since(t0);
    t0 = std::chrono::steady_clock::now();
    if (rc == GBRS_OK) rc = build_matrix(b, sc, rank, end.idx, end.col_ptr, s);
    *build_seconds += seconds_since(t0);
    bam_release_collected(b);
    end.R = b->num_reads;
    end.width = b->name_width;
    return rc;
}

std::string name_at(const std::vector<unsigned char> &bytes) {
    size_t n = bytes.size();
    while (n && bytes[n - 1] == 0) --n;
    return std::string((const char *)bytes.data(), n);
}

// GBRS_OK when both ends hold the same sorted distinct names; else the reference's sentence and the first sorted
// position at which they differ.  Of the two names there, the smaller one occurs in its own file only.
int check_pair_names(const gbrs_bam *fa, const PairEnd &a, const gbrs_bam *fb, const PairEnd &b, hipStream_t s) {
    const uint64_t R = std::min(a.R, b.R);
    const uint32_t W = (std::max(a.width, b.width) + 7) / 8;
    DevBuf<unsigned long long> first_diff;
    GBRS_TRY(first_diff.alloc(1));
    GBRS_HIP_CHECK(hipMemsetAsync(first_diff.p, 0xFF, sizeof(unsigned long long), s));
    hipLaunchKernelGGL(pair_names_differ_kernel, dim3(capped_grid(R * W)), dim3(256), 0, s, R, W, a.rname.p, a.width, b.rname.p,
                       b.width, first_diff.p);
    GBRS_HIP_CHECK(hipGetLastError());
    unsigned long long at = 0;
    GBRS_HIP_CHECK(hipMemcpyAsync(&at, first_diff.p, sizeof(at), hipMemcpyDeviceToHost, s));
    GBRS_HIP_CHECK(hipStreamSynchronize(s));
    if (at == ~0ull && a.R == b.R) return GBRS_OK;      // (equal names have equal lengths: the widths agree as well)
    const uint64_t p = std::min<uint64_t>(at, R);
    std::vector<unsigned char> na, nb;
    if (p < a.R) {
        na.resize(a.width);
        GBRS_HIP_CHECK(hipMemcpy(na.data(), a.rname.p + p * a.width, a.width, hipMemcpyDeviceToHost));
    }
    if (p < b.R) {
        nb.resize(b.width);
        GBRS_HIP_CHECK(hipMemcpy(nb.data(), b.rname.p + p * b.width, b.width, hipMemcpyDeviceToHost));
    }
    const std::string sa = name_at(na), sb = name_at(nb);
    const bool from_a = p >= b.R || (p < a.R && sa < sb);
    return fail(GBRS_ERR_INVALID,
                "The read ID's are not compatible. %s holds %llu reads and %s %llu; the sorted read names first differ at position "
                "%llu: '%s' is in %s only.",
                fa->path.c_str(), (unsigned long long)a.R, fb->path.c_str(), (unsigned long long)b.R, (unsigned long long)p,
                (from_a ? sa : sb).c_str(), (from_a ? fa : fb)->path.c_str());
}

// idx / col_ptr := the entries both ends have, in CSC order (idx stays unallocated when there is none)
int common_entries(const PairEnd &a, const PairEnd &b, uint64_t ncols, DevBuf<uint32_t> &idx, DevBuf<uint64_t> &col_ptr,
                   hipStream_t s) {
    GBRS_TRY(col_ptr.alloc(ncols + 1));
    const uint64_t n = a.idx.n;
    if (n == 0 || b.idx.n == 0) {
        GBRS_HIP_CHECK(hipMemsetAsync(col_ptr.p, 0, col_ptr.bytes(), s));
        return GBRS_OK;
    }
    Scratch sc;
    DevBuf<uint32_t> flag, pos;
    GBRS_TRY(flag.alloc(n + 1));
    GBRS_TRY(pos.alloc(n + 1));
    hipLaunchKernelGGL(pair_common_flag_kernel, dim3(capped_grid(n + 1)), dim3(256), 0, s, n, (uint32_t)ncols, a.col_ptr.p, a.idx.p,
                       b.col_ptr.p, b.idx.p, (uint64_t)b.idx.n, flag.p);
    GBRS_HIP_CHECK(hipGetLastError());
    GBRS_TRY(exclusive_scan(sc, flag.p, pos.p, n + 1, s));
    uint32_t n_common = 0;
    GBRS_HIP_CHECK(hipMemcpyAsync(&n_common, pos.p + n, sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    GBRS_HIP_CHECK(hipStreamSynchronize(s));
    if (n_common > n) return fail(GBRS_ERR_HIP, "internal error: more common entries than entries");
    if (n_common) {
        GBRS_TRY(idx.alloc(n_common));
        hipLaunchKernelGGL(pair_common_compact_kernel, dim3(capped_grid(n)), dim3(256), 0, s, n, a.idx.p, flag.p, pos.p,
                           (uint64_t)n_common, idx.p);
        GBRS_HIP_CHECK(hipGetLastError());
    }
    hipLaunchKernelGGL(pair_common_ptr_kernel, dim3(capped_grid(ncols + 1)), dim3(256), 0, s, ncols + 1, a.col_ptr.p, pos.p, n,
                       col_ptr.p);
    GBRS_HIP_CHECK(hipGetLastError());
    GBRS_HIP_CHECK(hipStreamSynchronize(s));
    return GBRS_OK;
}

// set := classes of (set's classes, then the addend's classes), weights = the two count vectors one after the other.
// The set's classes are distinct rows, so in first-seen order each keeps its id; an addend class equal to one of them
// adds its count there, the others follow in their own order - the first-occurrence order over the concatenated reads.
int merge_classes(CompressResult &set, CompressResult &add, uint32_t L, uint32_t H, hipStream_t s) {
    const uint64_t G1 = set.num_ecs, G2 = add.num_ecs, E1 = set.n_entries, E2 = add.n_entries, ncols = (uint64_t)H * L;
    if (G1 + G2 > 0xFFFFFFFFull) return fail(GBRS_ERR_UNSUPPORTED, "more than 2^32 - 1 equivalence classes to merge");
    DevBuf<uint32_t> idx;
    DevBuf<uint64_t> ptr;
    DevBuf<double> cnt;
    GBRS_TRY(idx.alloc(E1 + E2));
    GBRS_TRY(ptr.alloc(ncols + 1));
    GBRS_TRY(cnt.alloc(G1 + G2));
    hipLaunchKernelGGL(ecset_merge_ptr_kernel, dim3(capped_grid(ncols + 1)), dim3(256), 0, s, ncols + 1, set.col_ptr.p, add.col_ptr.p, ptr.p);
    GBRS_HIP_CHECK(hipGetLastError());
    if (E1) {
        hipLaunchKernelGGL(ecset_merge_copy_kernel, dim3(capped_grid(E1)), dim3(256), 0, s, E1, (uint32_t)ncols, set.col_ptr.p,
                           add.col_ptr.p, 0u, set.indices.p, 0u, E1 + E2, idx.p);
        GBRS_HIP_CHECK(hipGetLastError());
    }
    if (E2) {
        hipLaunchKernelGGL(ecset_merge_copy_kernel, dim3(capped_grid(E2)), dim3(256), 0, s, E2, (uint32_t)ncols, add.col_ptr.p,
                           set.col_ptr.p, 1u, add.indices.p, (uint32_t)G1, E1 + E2, idx.p);
        GBRS_HIP_CHECK(hipGetLastError());
    }
    GBRS_HIP_CHECK(hipMemcpyAsync(cnt.p, set.count.p, G1 * sizeof(double), hipMemcpyDeviceToDevice, s));
    GBRS_HIP_CHECK(hipMemcpyAsync(cnt.p + G1, add.count.p, G2 * sizeof(double), hipMemcpyDeviceToDevice, s));
    GBRS_HIP_CHECK(hipStreamSynchronize(s));
    add.indices.release();
    add.col_ptr.release();
    add.count.release();
    CompressResult merged;                       // the set stays as it is until the merge has succeeded
    GBRS_TRY(compress_device(merged, G1 + G2, L, H, E1 + E2, idx.p, ptr.p, cnt.p, s));
    set.num_ecs = merged.num_ecs;
    set.n_entries = merged.n_entries;
    set.col_ptr.swap(merged.col_ptr);
    set.indices.swap(merged.indices);
    set.count.swap(merged.count);
    return GBRS_OK;
}

}  // namespace
}  // namespace gbrs

struct gbrs_ecset {
    int device = 0;
    uint32_t L = 0, H = 0;
    uint64_t num_reads = 0;
    gbrs::CompressResult res;                    // num_ecs == 0: no file has been added
};

extern "C" {

int gbrs_bam_convert(gbrs_bam_t *b, int device, uint64_t *num_reads, uint32_t *name_width, uint64_t *nnz_per_hap,
                     double *stage_seconds) {
    using namespace gbrs;
    if (!b || !num_reads || !name_width || !nnz_per_hap) return fail(GBRS_ERR_INVALID, "bad argument");
    if (!b->map_set) return fail(GBRS_ERR_STATE, "gbrs_bam_set_reference_map has not been called");
    GBRS_TRY(select_device(device));          // before the file is read: without a device nothing else is worth doing
    if (b->dev && b->dev_free) b->dev_free(b->dev);
    b->dev = nullptr;
    b->converted = false;
    if ((uint64_t)b->num_haps * b->num_loci > 0xFFFFFFFFull)
        return fail(GBRS_ERR_UNSUPPORTED, "%u haplotypes x %u loci: more than 2^32 - 1 columns", b->num_haps, b->num_loci);
    RoctxRange range("gbrs_bam_convert");
    auto t0 = std::chrono::steady_clock::now();
    GBRS_TRY(bam_collect(b));
    if (stage_seconds) stage_seconds[0] = seconds_since(t0);
    const uint64_t C = b->cand_off.size() - 1;
    DevResult *res = new DevResult();
    res->device = device;
    b->dev = res;
    b->dev_free = free_result;
    int rc = GBRS_OK;
    b->num_reads = 0;
    b->name_width = 1;
    b->col_ptr.assign((uint64_t)b->num_haps * b->num_loci + 1, 0);
    if (stage_seconds) stage_seconds[1] = stage_seconds[2] = 0.0;
    if (C) {
        hipStream_t s = nullptr;
        Scratch sc;
        DevBuf<uint32_t> rank;
        DevBuf<uint64_t> col_ptr;
        t0 = std::chrono::steady_clock::now();
        rc = rank_names(b, sc, rank, &res->rname, s);
        if (stage_seconds) stage_seconds[1] = seconds_since(t0);
        t0 = std::chrono::steady_clock::now();
        if (rc == GBRS_OK) rc = build_matrix(b, sc, rank, res->idx, col_ptr, s);
        if (stage_seconds) stage_seconds[2] = seconds_since(t0);
    }
    bam_release_collected(b);
    if (rc != GBRS_OK) {
        free_result(res);
        b->dev = nullptr;
        return rc;
    }
    for (uint32_t h = 0; h < b->num_haps; ++h) {
        const uint64_t n = b->col_ptr[(uint64_t)(h + 1) * b->num_loci] - b->col_ptr[(uint64_t)h * b->num_loci];
        if (n > 0xFFFFFFFFull) {
            free_result(res);
            b->dev = nullptr;
            return fail(GBRS_ERR_UNSUPPORTED, "haplotype %u has %llu entries: more than uint32 index arrays hold", h, (unsigned long long)n);
        }
        nnz_per_hap[h] = n;
    }
    *num_reads = b->num_reads;
    *name_width = b->name_width;
    b->converted = true;
    return GBRS_OK;
}

int gbrs_bam_get(gbrs_bam_t *b, uint32_t *const *indptr_out, uint32_t *const *indices_out, char *rname_out) {
    using namespace gbrs;
    if (!b || !indptr_out || !indices_out) return fail(GBRS_ERR_INVALID, "bad argument");
    if (!b->converted || !b->dev) return fail(GBRS_ERR_STATE, "gbrs_bam_convert has not been run");
    DevResult *res = static_cast<DevResult *>(b->dev);
    GBRS_TRY(select_device(res->device));
    const uint64_t L = b->num_loci;
    for (uint32_t h = 0; h < b->num_haps; ++h) {
        const uint64_t base = b->col_ptr[h * L], n = b->col_ptr[(h + 1) * L] - base;
        if (!indptr_out[h] || (n && !indices_out[h])) return fail(GBRS_ERR_INVALID, "output buffer %u is NULL", h);
        for (uint64_t l = 0; l <= L; ++l) indptr_out[h][l] = (uint32_t)(b->col_ptr[h * L + l] - base);
        if (n) GBRS_HIP_CHECK(hipMemcpy(indices_out[h], res->idx.p + base, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    }
    if (rname_out && b->num_reads)
        GBRS_HIP_CHECK(hipMemcpy(rname_out, res->rname.p, b->num_reads * (uint64_t)b->name_width, hipMemcpyDeviceToHost));
    return GBRS_OK;
}

int gbrs_ecset_create(uint32_t num_loci, uint32_t num_haps, int device, gbrs_ecset_t **out) {
    using namespace gbrs;
    if (!out) return fail(GBRS_ERR_INVALID, "out is NULL");
    *out = nullptr;
    if (num_haps < 1 || num_haps > 16 || num_loci < 1 || num_loci >= (1u << 27))
        return fail(GBRS_ERR_INVALID, "compress needs 1 <= H <= 16 and 1 <= L < 2^27 loci");
    GBRS_TRY(select_device(device));
    gbrs_ecset *e = new gbrs_ecset();
    e->device = device;
    e->L = num_loci;
    e->H = num_haps;
    *out = e;
    return GBRS_OK;
}

int gbrs_ecset_add_bam(gbrs_ecset_t *e, gbrs_bam_t *b, uint64_t *num_reads_of_file, double *stage_seconds) {
    using namespace gbrs;
    if (!e || !b || !num_reads_of_file) return fail(GBRS_ERR_INVALID, "bad argument");
    if (!b->map_set) return fail(GBRS_ERR_STATE, "gbrs_bam_set_reference_map has not been called");
    if (b->num_loci != e->L || b->num_haps != e->H)
        return fail(GBRS_ERR_INVALID, "%s: the reference map has %u loci x %u haplotypes, the set %u x %u", b->path.c_str(),
                    b->num_loci, b->num_haps, e->L, e->H);
    GBRS_TRY(select_device(e->device));
    if (b->dev && b->dev_free) b->dev_free(b->dev);      // (an earlier gbrs_bam_convert: the handle keeps nothing on the device)
    b->dev = nullptr;
    b->converted = false;
    RoctxRange range("gbrs_ecset_add_bam");
    *num_reads_of_file = 0;
    if (stage_seconds) stage_seconds[0] = stage_seconds[1] = stage_seconds[2] = 0.0;
    auto t0 = std::chrono::steady_clock::now();
    GBRS_TRY(bam_collect(b));
    if (stage_seconds) stage_seconds[0] = seconds_since(t0);
    if (b->cand_off.size() < 2) {                        // no record at all: nothing to add
        bam_release_collected(b);
        return GBRS_OK;
    }
    hipStream_t s = nullptr;
    const uint64_t ncols = (uint64_t)e->H * e->L;
    CompressResult file;
    int rc = GBRS_OK;
    {
        Scratch sc;
        DevBuf<uint32_t> rank, idx;
        DevBuf<uint64_t> col_ptr;
        t0 = std::chrono::steady_clock::now();
        rc = rank_names(b, sc, rank, nullptr, s);
        if (stage_seconds) stage_seconds[1] = seconds_since(t0);
        t0 = std::chrono::steady_clock::now();
        if (rc == GBRS_OK) rc = build_matrix(b, sc, rank, idx, col_ptr, s);
        bam_release_collected(b);
        if (rc != GBRS_OK) return rc;
        rank.release();
        sc.buf.release();
        if (!col_ptr.p) {                                // no kept record: every read is in the empty class
            GBRS_TRY(col_ptr.alloc(ncols + 1));
            GBRS_HIP_CHECK(hipMemsetAsync(col_ptr.p, 0, col_ptr.bytes(), s));
        }
        GBRS_TRY(compress_device(file, b->num_reads, e->L, e->H, idx.n, idx.p, col_ptr.p, nullptr, s));
    }
    if (e->res.num_ecs == 0) {
        e->res.num_ecs = file.num_ecs;
        e->res.n_entries = file.n_entries;
        e->res.col_ptr.swap(file.col_ptr);
        e->res.indices.swap(file.indices);
        e->res.count.swap(file.count);
    } else {
        GBRS_TRY(merge_classes(e->res, file, e->L, e->H, s));
    }
    if (stage_seconds) stage_seconds[2] = seconds_since(t0);
    e->num_reads += b->num_reads;
    *num_reads_of_file = b->num_reads;
    return GBRS_OK;
}

int gbrs_ecset_add_bam_pair(gbrs_ecset_t *e, gbrs_bam_t *first, gbrs_bam_t *second, uint64_t *num_reads_of_pair,
                            double *stage_seconds) {
    using namespace gbrs;
    if (!e || !first || !second || !num_reads_of_pair) return fail(GBRS_ERR_INVALID, "bad argument");
    if (first == second) return fail(GBRS_ERR_INVALID, "the two ends of a pair need a handle each");
    gbrs_bam *ends[2] = {first, second};
    for (gbrs_bam *b : ends)
        if (!b->map_set) return fail(GBRS_ERR_STATE, "gbrs_bam_set_reference_map has not been called");
    for (gbrs_bam *b : ends)
        if (b->num_loci != e->L || b->num_haps != e->H)
            return fail(GBRS_ERR_INVALID, "%s: the reference map has %u loci x %u haplotypes, the set %u x %u", b->path.c_str(),
                        b->num_loci, b->num_haps, e->L, e->H);
    GBRS_TRY(select_device(e->device));
    for (gbrs_bam *b : ends) {                           // (an earlier gbrs_bam_convert: the handles keep nothing on the device)
        if (b->dev && b->dev_free) b->dev_free(b->dev);
        b->dev = nullptr;
        b->converted = false;
    }
    RoctxRange range("gbrs_ecset_add_bam_pair");
    *num_reads_of_pair = 0;
    double unused[4];
    double *secs = stage_seconds ? stage_seconds : unused;     // read, rank, common, classes (the matrices count as classes, as in add_bam)
    secs[0] = secs[1] = secs[2] = secs[3] = 0.0;
    hipStream_t s = nullptr;
    const uint64_t ncols = (uint64_t)e->H * e->L;
    auto t0 = std::chrono::steady_clock::now();
    int rc = bam_collect(first);
    secs[0] += seconds_since(t0);
    if (rc != GBRS_OK) return rc;
    const bool first_empty = first->cand_off.size() < 2;
    PairEnd a, b;
    if (first_empty) bam_release_collected(first);
    else {
        RoctxRange r("pair_first_end");
        GBRS_TRY(convert_end(first, a, &secs[1], &secs[3], s));
    }
    t0 = std::chrono::steady_clock::now();
    rc = bam_collect(second);
    secs[0] += seconds_since(t0);
    if (rc != GBRS_OK) return rc;
    const bool second_empty = second->cand_off.size() < 2;
    if (first_empty || second_empty) {
        bam_release_collected(second);
        if (first_empty && second_empty) return GBRS_OK; // no record at all in either end: nothing to add
        return fail(GBRS_ERR_INVALID, "The read ID's are not compatible. %s holds no record, %s does.",
                    (first_empty ? first : second)->path.c_str(), (first_empty ? second : first)->path.c_str());
    }
    {
        RoctxRange r("pair_second_end");
        GBRS_TRY(convert_end(second, b, &secs[1], &secs[3], s));
    }
    CompressResult file;
    {
        DevBuf<uint32_t> idx;
        DevBuf<uint64_t> col_ptr;
        t0 = std::chrono::steady_clock::now();
        {
            RoctxRange r("pair_common");
            rc = check_pair_names(first, a, second, b, s);
            a.rname.release();
            b.rname.release();
            if (rc == GBRS_OK) rc = common_entries(a, b, ncols, idx, col_ptr, s);
        }
        secs[2] = seconds_since(t0);
        if (rc != GBRS_OK) return rc;
        b.idx.release();
        b.col_ptr.release();
        a.idx.release();
        a.col_ptr.release();
        t0 = std::chrono::steady_clock::now();
        GBRS_TRY(compress_device(file, a.R, e->L, e->H, idx.n, idx.p, col_ptr.p, nullptr, s));
    }
    if (e->res.num_ecs == 0) {
        e->res.num_ecs = file.num_ecs;
        e->res.n_entries = file.n_entries;
        e->res.col_ptr.swap(file.col_ptr);
        e->res.indices.swap(file.indices);
        e->res.count.swap(file.count);
    } else {
        GBRS_TRY(merge_classes(e->res, file, e->L, e->H, s));
    }
    secs[3] += seconds_since(t0);
    e->num_reads += a.R;
    *num_reads_of_pair = a.R;
    return GBRS_OK;
}

int gbrs_ecset_sizes(gbrs_ecset_t *e, uint64_t *num_reads, uint64_t *num_ecs, uint64_t *nnz_per_hap) {
    using namespace gbrs;
    if (!e || !num_reads || !num_ecs || !nnz_per_hap) return fail(GBRS_ERR_INVALID, "bad argument");
    *num_reads = e->num_reads;
    *num_ecs = e->res.num_ecs;
    for (uint32_t h = 0; h < e->H; ++h) nnz_per_hap[h] = 0;
    if (e->res.num_ecs == 0) return GBRS_OK;
    GBRS_TRY(select_device(e->device));
    const uint64_t L = e->L;
    std::vector<uint64_t> cp((size_t)e->H * L + 1);
    GBRS_HIP_CHECK(hipMemcpy(cp.data(), e->res.col_ptr.p, cp.size() * sizeof(uint64_t), hipMemcpyDeviceToHost));
    for (uint32_t h = 0; h < e->H; ++h) nnz_per_hap[h] = cp[(h + 1) * L] - cp[h * L];
    return GBRS_OK;
}

int gbrs_ecset_get(gbrs_ecset_t *e, uint32_t *const *indptr_out, uint32_t *const *indices_out, double *count_out) {
    using namespace gbrs;
    if (!e || !indptr_out || !indices_out) return fail(GBRS_ERR_INVALID, "bad argument");
    const uint64_t L = e->L;
    for (uint32_t h = 0; h < e->H; ++h)
        if (!indptr_out[h]) return fail(GBRS_ERR_INVALID, "output buffer %u is NULL", h);
    if (e->res.num_ecs == 0) {
        for (uint32_t h = 0; h < e->H; ++h)
            for (uint64_t l = 0; l <= L; ++l) indptr_out[h][l] = 0;
        return GBRS_OK;
    }
    GBRS_TRY(select_device(e->device));
    std::vector<uint64_t> cp((size_t)e->H * L + 1);
    GBRS_HIP_CHECK(hipMemcpy(cp.data(), e->res.col_ptr.p, cp.size() * sizeof(uint64_t), hipMemcpyDeviceToHost));
    for (uint32_t h = 0; h < e->H; ++h) {
        const uint64_t base = cp[h * L], n = cp[(h + 1) * L] - base;
        if (n && !indices_out[h]) return fail(GBRS_ERR_INVALID, "output buffer %u is NULL", h);
        for (uint64_t l = 0; l <= L; ++l) indptr_out[h][l] = (uint32_t)(cp[h * L + l] - base);
        if (n) GBRS_HIP_CHECK(hipMemcpy(indices_out[h], e->res.indices.p + base, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    }
    if (count_out) GBRS_HIP_CHECK(hipMemcpy(count_out, e->res.count.p, e->res.num_ecs * sizeof(double), hipMemcpyDeviceToHost));
    return GBRS_OK;
}

int gbrs_ecset_destroy(gbrs_ecset_t *e) {
    if (e) {
        (void)hipSetDevice(e->device);
        delete e;
    }
    return GBRS_OK;
}

}  // extern "C"
