// Builds the packed-row-tile device layout (em_layout.h) from the reference's CSC arrays, entirely
// on the device.  rocPRIM provides the radix sorts and scans (setup plumbing, run once per
// handle); every transformation kernel is written here.
//
// Pipeline
//   entries (h, l, r)  --sort by (r, l, h)-->  (row, locus) pairs with a haplotype mask
//   rows  --sort by (first locus, hash of locus list, hash of masks)-->  similar rows adjacent
//   [optional] identical adjacent rows merged into one weighted row (what `gbrs compress` does)
//   tiles cut where a tile's words or its distinct ids reach their limit, sized for one round of the chip's workgroup
//   places (cut_tiles_exact); under a forced size or for a sample of several rounds: where the running count of words
//   or of the loci of distinct locus lists crosses a chunk border
//   per tile: locus dictionary (LDS bitonic sort + unique), rows padded so none straddles a
//   64-word batch, words emitted with dictionary-local indices
//   inverted index locus -> slots for the gather kernel
#include "em_layout.h"
#include "prim.h"

#include <algorithm>

namespace gbrs {
namespace {


// ---- kernels --------------------------------------------------------------------------------

struct BuildFlags {
    unsigned int duplicate;      // the same (row, locus, haplotype) stored twice
    unsigned int dict_overflow;  // a tile dictionary exceeded its capacity (internal error)
    unsigned int bad_row;        // row id >= R
    unsigned int n_long;         // rows with more than max_row_words(H) loci
    unsigned int long_pairs;     // their (row, locus) pairs: what the tiles do not hold
};

// Every wavefront takes a contiguous span of KEY_SPAN entries: one full search for the column of its
// first entry, after that columns only move forward (a column holds some hundreds of entries, so most
// 64-entry steps stay inside the current one).  A full search per 64 entries made this the slowest
// kernel of the build: two chains of ~20 dependent loads for every 64 keys.
constexpr int KEY_ITERS = 32, KEY_SPAN = 64 * KEY_ITERS;
__global__ void __launch_bounds__(256)
make_keys_kernel(uint64_t n, uint32_t ncols, uint32_t L, uint64_t R, unsigned row_shift,
                 const uint64_t *__restrict__ col_ptr, const uint32_t *__restrict__ ent_row,
                 uint64_t *__restrict__ keys, BuildFlags *flags, uint32_t view_h = 0) {
    // view_h > 0 (em_layout.h, "half-loci"): haplotype h of locus l is keyed as haplotype h % view_h of locus
    // l * (H / view_h) + h / view_h - the same element of the locus-major vectors under a narrower haplotype count
    // key = row << row_shift | locus << 5 | haplotype; row_shift = 32, or 5 + the locus bits so that a
    // radix sort of the used bits has no all-zero digit to pass over
    const int lane = threadIdx.x & 63;
    const uint64_t base = ((uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * KEY_SPAN;
    if (base >= n) return;
    uint32_t c = 0;
    if (lane == 0) c = find_column(col_ptr, 0, ncols - 1, base);
    c = __shfl(c, 0, WAVE);
    bool bad = false;
    for (int it = 0; it < KEY_ITERS; ++it) {
        const uint64_t kb = base + (uint64_t)it * 64;
        if (kb >= n) break;
        c = find_column_from(col_ptr, c, ncols, kb);              // uniform: the column of the step's first entry
        const uint64_t k = kb + lane;
        if (k >= n) continue;
        const uint32_t mine = col_ptr[c + 1] > min(kb + 63, n - 1) ? c : find_column_from(col_ptr, c, ncols, k);
        uint32_t h = mine / L, l = mine - h * L;
        if (view_h) {
            l = l * (ncols / L / view_h) + h / view_h;
            h = h % view_h;
        }
        const uint32_t r = ent_row[k];
        bad |= r >= R;
        keys[k] = ((uint64_t)r << row_shift) | ((uint64_t)l << 5) | h;
    }
    if (bad) flags->bad_row = 1;
}

__global__ void pair_flag_kernel(uint64_t n, const uint64_t *__restrict__ keys, uint32_t *__restrict__ flag,
                                 BuildFlags *flags) {
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    uint32_t f = 1;
    if (k > 0) {
        const uint64_t a = keys[k - 1], b = keys[k];
        if (a == b) flags->duplicate = 1;
        f = (a >> 5) != (b >> 5);
    }
    flag[k] = f;
}

__global__ void emit_pairs_kernel(uint64_t n, const uint64_t *__restrict__ keys, const uint32_t *__restrict__ flag,
                                  const uint32_t *__restrict__ pidx, unsigned row_shift,
                                  uint32_t *__restrict__ prow, uint32_t *__restrict__ ploc,
                                  uint32_t *__restrict__ pmask) {
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n || !flag[k]) return;
    const uint64_t key = keys[k];
    uint32_t mask = 0;
    for (uint64_t j = k; j < n && (keys[j] >> 5) == (key >> 5); ++j) mask |= 1u << (uint32_t)(keys[j] & 31);
    const uint32_t p = pidx[k];
    prow[p] = (uint32_t)(key >> row_shift);
    ploc[p] = (uint32_t)((key >> 5) & ((1u << (row_shift - 5)) - 1u));
    pmask[p] = mask;
}

__global__ void row_flag_kernel(uint64_t np, const uint32_t *__restrict__ prow, uint32_t *__restrict__ flag) {
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= np) return;
    flag[p] = (p == 0) || prow[p] != prow[p - 1];
}

__global__ void row_start_kernel(uint64_t np, uint64_t nrows, const uint32_t *__restrict__ flag,
                                 const uint32_t *__restrict__ ridx, const uint32_t *__restrict__ prow,
                                 uint32_t *__restrict__ rowstart, uint32_t *__restrict__ row_orig) {
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p == 0) rowstart[nrows] = (uint32_t)np;
    if (p >= np || !flag[p]) return;
    rowstart[ridx[p]] = (uint32_t)p;
    row_orig[ridx[p]] = prow[p];
}

// ---- locus sets (em_layout.h) ---------------------------------------------------------------------
constexpr uint32_t NO_SET = 0xFFFFFFFFu;
constexpr uint32_t SET_MAX_LOCI = 1024;

__device__ __forceinline__ uint64_t mix64(uint64_t h, uint64_t v) {
    h = (h ^ v) * 0x9E3779B97F4A7C15ull;
    return h ^ (h >> 29);
}

// flag[r] = 1 when row r has >= 2 (row, locus) pairs that all carry one mask; key[r] = hash of its locus list
__global__ void set_candidate_kernel(uint64_t nrows, const uint32_t *__restrict__ rowstart, const uint32_t *__restrict__ ploc,
                                     const uint32_t *__restrict__ pmask, uint64_t *__restrict__ key, uint32_t *__restrict__ flag) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= nrows) return;
    const uint32_t b = rowstart[r], e = rowstart[r + 1];
    bool ok = e - b >= 2 && e - b <= SET_MAX_LOCI;
    uint64_t h = e - b;
    if (ok) {
        const uint32_t m0 = pmask[b];
        for (uint32_t k = b; k < e; ++k) {
            ok &= pmask[k] == m0;
            h = mix64(h, ploc[k]);
        }
    }
    flag[r] = ok ? 1u : 0u;
    key[r] = h;
}

__global__ void set_compact_kernel(uint64_t nrows, const uint32_t *__restrict__ flag, const uint32_t *__restrict__ cidx,
                                   const uint64_t *__restrict__ key, uint64_t *__restrict__ ckey, uint32_t *__restrict__ crow) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= nrows || !flag[r]) return;
    ckey[cidx[r]] = key[r];
    crow[cidx[r]] = (uint32_t)r;
}

// candidates sorted by hash: head[i] = 1 when candidate i's locus list differs from its predecessor's (exact comparison:
// a hash collision can only split a set in two, never join two)
__global__ void set_head_kernel(uint64_t nc, const uint64_t *__restrict__ skey, const uint32_t *__restrict__ srow,
                                const uint32_t *__restrict__ rowstart, const uint32_t *__restrict__ ploc, uint32_t *__restrict__ head) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nc) return;
    bool same = i > 0 && skey[i] == skey[i - 1];
    if (same) {
        const uint32_t a = srow[i], b = srow[i - 1];
        const uint32_t a0 = rowstart[a], b0 = rowstart[b], n = rowstart[a + 1] - a0;
        same = n == rowstart[b + 1] - b0;
        for (uint32_t k = 0; same && k < n; ++k) same = ploc[a0 + k] == ploc[b0 + k];
    }
    head[i] = same ? 0u : 1u;
}

__global__ void set_assign_kernel(uint64_t nc, const uint32_t *__restrict__ head, const uint32_t *__restrict__ hincl,
                                  const uint32_t *__restrict__ srow, const uint32_t *__restrict__ rowstart,
                                  uint32_t *__restrict__ set_of_row, uint32_t *__restrict__ set_len, uint32_t *__restrict__ set_rep) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nc) return;
    const uint32_t k = hincl[i] - 1, r = srow[i];
    set_of_row[r] = k;
    if (head[i]) {
        set_len[k] = rowstart[r + 1] - rowstart[r];
        set_rep[k] = r;
    }
}

__global__ void set_members_kernel(uint32_t n_sets, const uint32_t *__restrict__ set_ptr, const uint32_t *__restrict__ set_rep,
                                   const uint32_t *__restrict__ rowstart, const uint32_t *__restrict__ ploc,
                                   uint32_t *__restrict__ members) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_sets) return;
    const uint32_t b = rowstart[set_rep[k]], o = set_ptr[k], n = set_ptr[k + 1] - o;
    for (uint32_t j = 0; j < n; ++j) members[o + j] = ploc[b + j];
}

__global__ void set_row_len_kernel(uint64_t nrows, const uint32_t *__restrict__ rowstart, const uint32_t *__restrict__ set_of_row,
                                   uint32_t *__restrict__ newlen) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= nrows) return;
    newlen[r] = set_of_row[r] != NO_SET ? 1u : rowstart[r + 1] - rowstart[r];
}

__global__ void set_rewrite_kernel(uint64_t nrows, uint32_t L, const uint32_t *__restrict__ rowstart,
                                   const uint32_t *__restrict__ set_of_row, const uint32_t *__restrict__ newstart,
                                   const uint32_t *__restrict__ ploc, const uint32_t *__restrict__ pmask,
                                   uint32_t *__restrict__ ploc2, uint32_t *__restrict__ pmask2) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= nrows) return;
    const uint32_t b = rowstart[r], e = rowstart[r + 1], o = newstart[r], k = set_of_row[r];
    if (k != NO_SET) {
        ploc2[o] = L + k;
        pmask2[o] = pmask[b];
    } else {
        for (uint32_t j = b; j < e; ++j) {
            ploc2[o + (j - b)] = ploc[j];
            pmask2[o + (j - b)] = pmask[j];
        }
    }
}

// ---- locus sets per mask group (round 4) ----------------------------------------------------------------------------
// A read that aligns to several isoforms of a gene with DIFFERENT haplotype masks is no whole-row set, but the loci of the row
// that share a mask are one: den = sum over the groups g of sum_h m_g,h * (theta[l1,h] + theta[l2,h] + ...), and every locus of a
// group receives the same count/den.  Rows are regrouped by (mask, locus); every group of >= 2 loci is a candidate, and a
// candidate becomes a set only when at least `min_rows` rows carry it: thin sets fill the tiles' dictionaries for nothing
// (profiles/r03_estep_experiments.txt item 16: 216 k sets, most of them carried by a handful of reads, made the
// multi-isoform sample 1.8x slower; the frequent ones are where the reads are).
constexpr uint32_t GROUP_ROW_MAX = 32;

// per row: pairs sorted by (mask, locus) into gloc / gmask (same offsets); nseg[r] = number of mask groups
__global__ void group_sort_kernel(uint64_t nrows, const uint32_t *__restrict__ rowstart, const uint32_t *__restrict__ ploc,
                                  const uint32_t *__restrict__ pmask, uint32_t *__restrict__ gloc, uint32_t *__restrict__ gmask,
                                  uint32_t *__restrict__ nseg) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= nrows) return;
    const uint32_t b = rowstart[r], n = rowstart[r + 1] - b;
    if (n > GROUP_ROW_MAX) {                     // long rows stay as they are: every pair a group of its own
        for (uint32_t k = 0; k < n; ++k) { gloc[b + k] = ploc[b + k]; gmask[b + k] = pmask[b + k]; }
        nseg[r] = n;
        return;
    }
    uint64_t v[GROUP_ROW_MAX];
    for (uint32_t k = 0; k < n; ++k) v[k] = ((uint64_t)pmask[b + k] << 32) | ploc[b + k];
    for (uint32_t i = 1; i < n; ++i) {           // insertion sort (the loci arrive ascending: only the masks reorder)
        const uint64_t x = v[i];
        uint32_t j = i;
        while (j > 0 && v[j - 1] > x) { v[j] = v[j - 1]; --j; }
        v[j] = x;
    }
    uint32_t ns = 0;
    for (uint32_t k = 0; k < n; ++k) {
        gloc[b + k] = (uint32_t)v[k];
        gmask[b + k] = (uint32_t)(v[k] >> 32);
        ns += (k == 0 || (v[k] >> 32) != (v[k - 1] >> 32)) ? 1u : 0u;
    }
    nseg[r] = ns;
}

// per row: its groups as segments [seg_begin, seg_begin + seg_len) of gloc; a group of >= 2 loci is a candidate with the hash
// of its locus list as key
__global__ void group_segments_kernel(uint64_t nrows, const uint32_t *__restrict__ rowstart, const uint32_t *__restrict__ gloc,
                                      const uint32_t *__restrict__ gmask, const uint32_t *__restrict__ segoff,
                                      uint32_t *__restrict__ seg_begin, uint32_t *__restrict__ seg_len, uint64_t *__restrict__ key,
                                      uint32_t *__restrict__ cand) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= nrows) return;
    const uint32_t b = rowstart[r], e = rowstart[r + 1];
    uint32_t s = segoff[r];
    const bool plain = e - b > GROUP_ROW_MAX;
    uint32_t k = b;
    while (k < e) {
        uint32_t k2 = k + 1;
        uint64_t h = 0;
        if (!plain) {
            h = mix64(0x51ed270b1ull, gloc[k]);
            while (k2 < e && gmask[k2] == gmask[k]) { h = mix64(h, gloc[k2]); ++k2; }
        }
        seg_begin[s] = k;
        seg_len[s] = k2 - k;
        key[s] = mix64(h, k2 - k);
        cand[s] = k2 - k >= 2 ? 1u : 0u;
        ++s;
        k = k2;
    }
}

__global__ void group_compact_kernel(uint64_t nseg, const uint32_t *__restrict__ cand, const uint32_t *__restrict__ cidx,
                                     const uint64_t *__restrict__ key, uint64_t *__restrict__ ckey, uint32_t *__restrict__ cseg) {
    const uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= nseg || !cand[s]) return;
    ckey[cidx[s]] = key[s];
    cseg[cidx[s]] = (uint32_t)s;
}

// candidates sorted by hash: head[i] = 1 when candidate i's locus list differs from its predecessor's (exact comparison)
__global__ void group_head_kernel(uint64_t nc, const uint64_t *__restrict__ skey, const uint32_t *__restrict__ sseg,
                                  const uint32_t *__restrict__ seg_begin, const uint32_t *__restrict__ seg_len,
                                  const uint32_t *__restrict__ gloc, uint32_t *__restrict__ head) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nc) return;
    bool same = i > 0 && skey[i] == skey[i - 1];
    if (same) {
        const uint32_t a = sseg[i], b = sseg[i - 1];
        const uint32_t a0 = seg_begin[a], b0 = seg_begin[b], n = seg_len[a];
        same = n == seg_len[b];
        for (uint32_t k = 0; same && k < n; ++k) same = gloc[a0 + k] == gloc[b0 + k];
    }
    head[i] = same ? 0u : 1u;
}

// rows per provisional set, and its first candidate (sorted order) as representative
__global__ void group_count_kernel(uint64_t nc, const uint32_t *__restrict__ head, const uint32_t *__restrict__ hincl,
                                   const uint32_t *__restrict__ sseg, uint32_t *__restrict__ count, uint32_t *__restrict__ rep) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nc) return;
    const uint32_t k = hincl[i] - 1;
    atomicAdd(&count[k], 1u);
    if (head[i]) rep[k] = sseg[i];
}

__global__ void group_keep_kernel(uint32_t nprov, uint32_t min_rows, const uint32_t *__restrict__ count, uint32_t *__restrict__ keep) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < nprov) keep[k] = count[k] >= min_rows ? 1u : 0u;
}

// set_of_seg for the candidates of kept sets; length and representative segment of every kept set
__global__ void group_assign_kernel(uint64_t nc, const uint32_t *__restrict__ hincl, const uint32_t *__restrict__ sseg,
                                    const uint32_t *__restrict__ keep, const uint32_t *__restrict__ newid,
                                    const uint32_t *__restrict__ rep, const uint32_t *__restrict__ seg_len,
                                    uint32_t *__restrict__ set_of_seg, uint32_t *__restrict__ set_len, uint32_t *__restrict__ set_rep) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nc) return;
    const uint32_t k = hincl[i] - 1;
    if (!keep[k]) return;
    const uint32_t id = newid[k];
    set_of_seg[sseg[i]] = id;
    if (rep[k] == sseg[i]) {
        set_len[id] = seg_len[sseg[i]];
        set_rep[id] = sseg[i];
    }
}

__global__ void group_members_kernel(uint32_t n_sets, const uint32_t *__restrict__ set_ptr, const uint32_t *__restrict__ set_rep,
                                     const uint32_t *__restrict__ seg_begin, const uint32_t *__restrict__ gloc,
                                     uint32_t *__restrict__ members) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n_sets) return;
    const uint32_t b = seg_begin[set_rep[k]], o = set_ptr[k], n = set_ptr[k + 1] - o;
    for (uint32_t j = 0; j < n; ++j) members[o + j] = gloc[b + j];       // ascending: a group is sorted by locus
}

__global__ void group_row_len_kernel(uint64_t nrows, const uint32_t *__restrict__ segoff, const uint32_t *__restrict__ seg_len,
                                     const uint32_t *__restrict__ set_of_seg, uint32_t *__restrict__ newlen) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= nrows) return;
    uint32_t n = 0;
    for (uint32_t s = segoff[r]; s < segoff[r + 1]; ++s) n += set_of_seg[s] != NO_SET ? 1u : seg_len[s];
    newlen[r] = n;
}

// the rows in their new form: a kept group becomes one pair on its set's id, the others keep their pairs; ids ascending
__global__ void group_rewrite_kernel(uint64_t nrows, uint32_t L, const uint32_t *__restrict__ segoff,
                                     const uint32_t *__restrict__ seg_begin, const uint32_t *__restrict__ seg_len,
                                     const uint32_t *__restrict__ set_of_seg, const uint32_t *__restrict__ newstart,
                                     const uint32_t *__restrict__ gloc, const uint32_t *__restrict__ gmask,
                                     uint32_t *__restrict__ ploc2, uint32_t *__restrict__ pmask2) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= nrows) return;
    const uint32_t o = newstart[r], n = newstart[r + 1] - o;
    uint32_t w = o;
    for (uint32_t s = segoff[r]; s < segoff[r + 1]; ++s) {
        const uint32_t b = seg_begin[s], k = set_of_seg[s];
        if (k != NO_SET) {
            ploc2[w] = L + k;
            pmask2[w] = gmask[b];
            ++w;
        } else {
            for (uint32_t j = 0; j < seg_len[s]; ++j) { ploc2[w] = gloc[b + j]; pmask2[w] = gmask[b + j]; ++w; }
        }
    }
    if (n > GROUP_ROW_MAX) return;               // (a long row was copied in its own order)
    for (uint32_t i = 1; i < n; ++i) {           // back to ascending ids, as every later step expects of a row
        const uint32_t xl = ploc2[o + i], xm = pmask2[o + i];
        uint32_t j = i;
        while (j > 0 && ploc2[o + j - 1] > xl) { ploc2[o + j] = ploc2[o + j - 1]; pmask2[o + j] = pmask2[o + j - 1]; --j; }
        ploc2[o + j] = xl;
        pmask2[o + j] = xm;
    }
}


__device__ __forceinline__ uint32_t mix32(uint32_t h, uint32_t v) {
    h ^= v + 0x9e3779b9u + (h << 6) + (h >> 2);
    h *= 0x85ebca6bu;
    h ^= h >> 13;
    return h;
}

__global__ void row_key_kernel(uint64_t nrows, uint32_t max_row, unsigned loc_shift, const uint32_t *__restrict__ rowstart,
                               const uint32_t *__restrict__ ploc, const uint32_t *__restrict__ pmask,
                               uint64_t *__restrict__ key, uint32_t *__restrict__ ident, BuildFlags *flags) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= nrows) return;
    ident[r] = (uint32_t)r;
    const uint32_t a = rowstart[r], b = rowstart[r + 1];
    if (b - a > max_row) {
        key[r] = ~0ull;
        atomicAdd(&flags->n_long, 1u);
        atomicAdd(&flags->long_pairs, b - a);
        return;
    }
    uint32_t hl = 0x811c9dc5u, hm = 0x01000193u;
    for (uint32_t p = a; p < b; ++p) {
        hl = mix32(hl, ploc[p]);
        hm = mix32(hm, pmask[p]);
    }
    const uint64_t primary = (ploc[a] >> loc_shift) & 0xFFFFFFu;
    uint64_t k = (primary << 40) | ((uint64_t)(hl & 0xFFFFFFu) << 16) | (hm & 0xFFFFu);
    if (k == ~0ull) k -= 1;
    key[r] = k;
}

__device__ __forceinline__ bool same_loci(const uint32_t *__restrict__ rowstart, const uint32_t *__restrict__ ploc,
                                          uint32_t ra, uint32_t rb) {
    const uint32_t a = rowstart[ra], na = rowstart[ra + 1] - a;
    const uint32_t b = rowstart[rb], nb = rowstart[rb + 1] - b;
    if (na != nb) return false;
    for (uint32_t j = 0; j < na; ++j)
        if (ploc[a + j] != ploc[b + j]) return false;
    return true;
}

// head[i] = 1 when sorted row i starts a new (merged) row.  merge = 1: identical rows join; merge = 2 (the fold of identical
// one-word reads, em_layout.h): rows join only when both are exactly one (locus, mask) pair and the pairs are equal;
// merge = 3: the same, and rows that are both exactly two (locus, mask) pairs and equal pair for pair join too
__global__ void merge_flag_kernel(uint64_t n, int merge, const uint64_t *__restrict__ skey,
                                  const uint32_t *__restrict__ srow, const uint32_t *__restrict__ rowstart,
                                  const uint32_t *__restrict__ ploc, const uint32_t *__restrict__ pmask,
                                  uint32_t *__restrict__ head) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t f = 1;
    if (merge >= 2 && i > 0 && skey[i] == skey[i - 1]) {
        const uint32_t ra = srow[i - 1], rb = srow[i];
        const uint32_t a = rowstart[ra], b = rowstart[rb];
        const uint32_t na = rowstart[ra + 1] - a, nb = rowstart[rb + 1] - b;
        if (na == 1u && nb == 1u && ploc[a] == ploc[b] && pmask[a] == pmask[b]) f = 0;
        if (merge == 3 && na == 2u && nb == 2u && ploc[a] == ploc[b] && pmask[a] == pmask[b] && ploc[a + 1] == ploc[b + 1] &&
            pmask[a + 1] == pmask[b + 1])
            f = 0;
    } else if (merge == 1 && i > 0 && skey[i] == skey[i - 1]) {
        const uint32_t ra = srow[i - 1], rb = srow[i];
        if (same_loci(rowstart, ploc, ra, rb)) {
            const uint32_t a = rowstart[ra], b = rowstart[rb], cnt = rowstart[ra + 1] - a;
            bool eq = true;
            for (uint32_t j = 0; j < cnt; ++j) eq &= pmask[a + j] == pmask[b + j];
            if (eq) f = 0;
        }
    }
    head[i] = f;
}

// The fold's runs are cut every `cap` rows (what a word's count field holds): hpos is the position of the last head at or
// before row i (a max-scan of run_head_pos_kernel's output), and every cap-th row of a run becomes a head of its own
__global__ void run_head_pos_kernel(uint64_t n, const uint32_t *__restrict__ head, uint32_t *__restrict__ pos) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) pos[i] = head[i] ? (uint32_t)i : 0u;
}

__global__ void run_cut_kernel(uint64_t n, uint32_t cap, const uint32_t *__restrict__ hpos, uint32_t *__restrict__ head) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && ((uint32_t)i - hpos[i]) % cap == 0u) head[i] = 1u;
}

// the fold's two-word reads that lost their words to a neighbour (after the cut): one atomic per wavefront
__global__ void folded_two_kernel(uint64_t n, const uint32_t *__restrict__ head, const uint32_t *__restrict__ srow,
                                  const uint32_t *__restrict__ rowstart, unsigned long long *__restrict__ total) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool mine = false;
    if (i < n && !head[i]) {
        const uint32_t r = srow[i];
        mine = rowstart[r + 1] - rowstart[r] == 2u;
    }
    const unsigned long long b = __ballot(mine);
    if ((threadIdx.x & 63) == 0 && b != 0) atomicAdd(total, (unsigned long long)__popcll(b));
}

// per sorted row: merged ordinal m = incl[i] - 1; accumulate weights (merge) or the repeat count (fold), record representative
__global__ void merged_rows_kernel(uint64_t n, const uint32_t *__restrict__ head, const uint32_t *__restrict__ hincl,
                                   const uint32_t *__restrict__ srow, const uint32_t *__restrict__ row_orig,
                                   const double *__restrict__ count, uint32_t *__restrict__ hrow,
                                   double *__restrict__ weight, uint32_t *__restrict__ repeat) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t m = hincl[i] - 1;
    if (head[i]) hrow[m] = srow[i];
    if (repeat) atomicAdd(&repeat[m], 1u);
    if (weight) atomicAdd(&weight[m], count ? count[row_orig[srow[i]]] : 1.0);
}

__global__ void row_len_kernel(uint64_t m_rows, const uint32_t *__restrict__ hrow, const uint32_t *__restrict__ rowstart,
                               const uint32_t *__restrict__ ploc, uint32_t *__restrict__ npm,
                               uint32_t *__restrict__ dnew) {
    const uint64_t m = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= m_rows) return;
    const uint32_t r = hrow[m];
    const uint32_t cnt = rowstart[r + 1] - rowstart[r];
    npm[m] = cnt;
    const bool newlist = (m == 0) || !same_loci(rowstart, ploc, hrow[m - 1], r);
    dnew[m] = newlist ? cnt : 0;
}

__global__ void tile_flag_kernel(uint64_t m_rows, uint32_t tile_words, uint32_t dseg, const uint32_t *__restrict__ npm,
                                 const uint32_t *__restrict__ wordoff, const uint32_t *__restrict__ dincl,
                                 uint32_t *__restrict__ tflag) {
    const uint64_t m = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= m_rows) return;
    uint32_t f = 1;
    if (m > 0) {
        const uint32_t dc = dincl[m] - npm[m], dp = dincl[m - 1] - npm[m - 1];
        f = (wordoff[m] / tile_words != wordoff[m - 1] / tile_words) || (dc / dseg != dp / dseg);
    }
    tflag[m] = f;
}

// ---- the exact cut (cut_tiles_exact) ----
// ids of row m that the row before it does not have: a tile of rows a .. b holds at most npm[a] + the sum of these over
// a + 1 .. b distinct ids (an id's first row in the tile is a, or a row whose predecessor lacks it).  The rows are sorted
// by locus list, so the list (l1, l2) behind l1's single-locus reads counts l2 alone - row_len_kernel's dnew counts both
__global__ void row_new_ids_kernel(uint64_t m_rows, const uint32_t *__restrict__ hrow, const uint32_t *__restrict__ rowstart,
                                   const uint32_t *__restrict__ ploc, uint32_t *__restrict__ fresh) {
    const uint64_t m = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= m_rows) return;
    const uint32_t r = hrow[m], p0 = rowstart[r], p1 = rowstart[r + 1];
    uint32_t n = p1 - p0;
    if (m > 0) {
        const uint32_t q = hrow[m - 1], q0 = rowstart[q], q1 = rowstart[q + 1];
        for (uint32_t p = p0; p < p1; ++p) {
            const uint32_t id = ploc[p];
            for (uint32_t k = q0; k < q1; ++k)
                if (ploc[k] == id) { --n; break; }
        }
    }
    fresh[m] = n;
}

// candidates: a new one where the word offset passes a multiple of tile_words
__global__ void cand_flag_kernel(uint64_t m_rows, uint32_t tile_words, const uint32_t *__restrict__ wordoff,
                                 uint32_t *__restrict__ cflag) {
    const uint64_t m = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= m_rows) return;
    cflag[m] = (m == 0 || wordoff[m] / tile_words != wordoff[m - 1] / tile_words) ? 1u : 0u;
}

// distinct ids per candidate from the sorted (candidate, id) keys and their head flags
__global__ void cand_count_kernel(uint64_t n, const uint64_t *__restrict__ skeys, const uint32_t *__restrict__ flag,
                                  uint32_t *__restrict__ cnt) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && flag[i]) atomicAdd(&cnt[skeys[i] >> 32], 1u);
}

// a candidate whose distinct ids fit d_max is a tile; any other is split where the running count of fresh ids passes a
// multiple of dseg: the rows between two such lines bring fewer than dseg fresh ids, the first of them at most a row's
// words more - below d_max = dseg + max_row_words whatever the tile's first row is
__global__ void cut_flag_kernel(uint64_t m_rows, uint32_t dseg, uint32_t d_max, const uint32_t *__restrict__ cflag,
                                const uint32_t *__restrict__ cincl, const uint32_t *__restrict__ cnt,
                                const uint32_t *__restrict__ fincl, uint32_t *__restrict__ tflag) {
    const uint64_t m = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= m_rows) return;
    uint32_t f = cflag[m];
    if (!f && cnt[cincl[m] - 1] > d_max) f = fincl[m] / dseg != fincl[m - 1] / dseg;
    tflag[m] = f;
}

// interleave: rows of one locus list are dealt round-robin against the other lists of the tile so
// that the 64 words of a batch spread over as many dictionary entries as possible (LDS atomic
// conflicts in the E-step come from lanes that share a partial-sum copy AND a locus)
__global__ void group_flag_kernel(uint64_t m_rows, const uint32_t *__restrict__ dnew, const uint32_t *__restrict__ tflag,
                                  uint32_t *__restrict__ gflag, uint32_t *__restrict__ gpos) {
    const uint64_t m = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= m_rows) return;
    const uint32_t f = (dnew[m] > 0) || tflag[m];
    gflag[m] = f;
    gpos[m] = f ? (uint32_t)m : 0u;
}

__global__ void interleave_key_kernel(uint64_t m_rows, const uint32_t *__restrict__ tincl, const uint32_t *__restrict__ gstart,
                                      const uint32_t *__restrict__ gord, uint64_t *__restrict__ key,
                                      uint32_t *__restrict__ ident) {
    const uint64_t m = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= m_rows) return;
    const uint64_t rank = (uint32_t)m - gstart[m];
    key[m] = ((uint64_t)(tincl[m] - 1) << 40) | ((rank & 0x3FFFu) << 26) | (gord[m] & 0x3FFFFFFu);
    ident[m] = (uint32_t)m;
}

// stream order: inside a tile, rows by length (then in their sorted order), see tile_pad_kernel
__global__ void stream_key_kernel(uint64_t m_rows, const uint32_t *__restrict__ tincl, const uint32_t *__restrict__ npm,
                                  uint64_t *__restrict__ key, uint32_t *__restrict__ ident) {
    const uint64_t m = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= m_rows) return;
    key[m] = ((uint64_t)(tincl[m] - 1) << 40) | ((uint64_t)min(npm[m], 63u) << 32) | (uint32_t)m;
    ident[m] = (uint32_t)m;
}

__global__ void permute_rows_kernel(uint64_t m_rows, const uint32_t *__restrict__ perm, const uint32_t *__restrict__ hrow,
                                    const uint32_t *__restrict__ npm, const double *__restrict__ weight,
                                    const uint32_t *__restrict__ repeat, uint32_t *__restrict__ hrow2,
                                    uint32_t *__restrict__ npm2, double *__restrict__ weight2,
                                    uint32_t *__restrict__ repeat2) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= m_rows) return;
    const uint32_t m = perm[i];
    hrow2[i] = hrow[m];
    npm2[i] = npm[m];
    if (weight) weight2[i] = weight[m];
    if (repeat) repeat2[i] = repeat[m];
}

__global__ void tile_start_kernel(uint64_t m_rows, uint64_t n_tiles, const uint32_t *__restrict__ tflag,
                                  const uint32_t *__restrict__ tincl, uint32_t *__restrict__ tile_row) {
    const uint64_t m = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (m == 0) tile_row[n_tiles] = (uint32_t)m_rows;
    if (m >= m_rows || !tflag[m]) return;
    tile_row[tincl[m] - 1] = (uint32_t)m;
}

// Stripes (em_plan.h): head[m] = 1 when row m - a one- or two-word row, in the tiles' stream order - does not continue the
// group of the row before it: another length, another first id or, in a two-word row, another second id.  (Rows of one
// group are neighbours in that order up to a collision of the row key's hashes, which only makes two groups of one.)
__global__ void stripe_head_kernel(uint64_t m_rows, const uint32_t *__restrict__ npm, const uint32_t *__restrict__ hrow,
                                   const uint32_t *__restrict__ rowstart, const uint32_t *__restrict__ ploc,
                                   uint8_t *__restrict__ head) {
    const uint64_t m = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= m_rows) return;
    const uint32_t cnt = npm[m];
    uint8_t h = 1;
    if (m > 0 && cnt <= 2u && npm[m - 1] == cnt) {
        const uint32_t a = rowstart[hrow[m - 1]], b = rowstart[hrow[m]];
        h = (ploc[a] != ploc[b] || (cnt == 2u && ploc[a + 1] != ploc[b + 1])) ? 1 : 0;
    }
    head[m] = h;
}

// cells of a run of n rows whose groups (head) each start at a multiple of S and take whole stripes of S cells
__device__ __forceinline__ uint32_t stripe_cells(const uint8_t *__restrict__ head, uint32_t n, uint32_t S) {
    uint32_t c = 0;
    for (uint32_t k = 0; k < n; ++k) {
        if (head[k]) c = (c + S - 1u) & ~(S - 1u);
        ++c;
    }
    return (c + S - 1u) & ~(S - 1u);
}

// one thread per tile: padded offset of every row so that no row straddles a 64-word batch.
// streams: the tile's rows arrive grouped by length; a run of n rows of length w (w | 64) takes
// B = ceil(n / (64/w)) whole batches in which lane group g (w lanes) holds rows g*B .. g*B+B-1 of the
// run at batches 0 .. B-1: whichever batches a wavefront owns, each of its lanes walks a
// contiguous piece of the sorted rows.
// n_one[t]: the batches of the tile's run of one-word rows - the rows sort by length, so they are the tile's first
// (TileHdr::n_one); 0 in the other row orders.  n_two[t]: the batches of the run of two-word rows when it starts exactly at
// batch n_one[t] (TileHdr::n_two; the caller clears it for the layouts whose kernels do not read counts).
// head (stripes, em_plan.h; null: none): those two runs are laid out in CELLS - a group of rows starts at a cell that is a
// multiple of the run's stripe S and its last stripe is filled up with empty cells, B is rounded up to a multiple of S, and
// cell c sits on lane group c / B at batch c % B as a row of the plain run does.  A lane group therefore changes id only at
// batches that are a multiple of S from the run's first, and an empty cell has a word of its own group above it on its
// lane (fill_one_word_cells_kernel).  S is chosen per tile and run by em_stripe_pick; S = 0 is the plain placement.
__global__ void tile_pad_kernel(uint64_t n_tiles, int streams, const uint32_t *__restrict__ tile_row,
                                const uint32_t *__restrict__ npm, uint32_t *__restrict__ rowpad,
                                uint32_t *__restrict__ nbatch, uint32_t *__restrict__ n_one, uint32_t *__restrict__ n_two,
                                const uint8_t *__restrict__ head, int stripes_one, int stripes_two) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_tiles) return;
    uint32_t off = 0, one = 0, two = 0;
    const uint32_t end = tile_row[t + 1];
    uint32_t m = tile_row[t];
    while (m < end) {
        const uint32_t cnt = npm[m];
        if (streams && cnt <= 32u && (64u % cnt) == 0u) {
            uint32_t e = m + 1;
            while (e < end && npm[e] == cnt) ++e;
            const uint32_t n = e - m, G = 64u / cnt;
            uint32_t B = (n + G - 1) / G;
            off = (off + 63u) & ~63u;
            const bool lead_one = cnt == 1u && off == 0u, lead_two = cnt == 2u && off == one * 64u;
            uint32_t S = 0;
            if (head && (lead_one || lead_two)) {
                const int forced = lead_one ? stripes_one : stripes_two;
                S = forced >= 0 ? (uint32_t)forced : em_stripe_pick(forced, n, stripe_cells(head + m, n, 4u), stripe_cells(head + m, n, 2u));
            }
            if (S != 0u) {
                B = (stripe_cells(head + m, n, S) + G - 1) / G;
                B = (B + S - 1u) & ~(S - 1u);
                uint32_t c = 0;
                for (uint32_t k = 0; k < n; ++k) {
                    if (head[m + k]) c = (c + S - 1u) & ~(S - 1u);
                    rowpad[m + k] = off + (c % B) * 64u + (c / B) * cnt;
                    ++c;
                }
            } else {
                for (uint32_t k = 0; k < n; ++k) rowpad[m + k] = off + (k % B) * 64u + (k / B) * cnt;
            }
            if (lead_one) one = B;
            if (lead_two) two = B;
            off += B * 64u;
            m = e;
        } else {
            if ((off & 63u) + cnt > 64u) off = (off + 63u) & ~63u;
            rowpad[m] = off;
            off += cnt;
            ++m;
        }
    }
    nbatch[t] = (off + 63u) >> 6;
    n_one[t] = one;
    n_two[t] = two;
}

// Per-tile dictionaries = the distinct loci (and locus sets) of a tile's rows, ascending.  Built from ONE radix sort of
// (tile, id) keys over all the pairs of the layout (round 4; before: a bitonic sort per tile in LDS, which capped a tile at
// 16,384 words - and the E-step likes its tiles as large as one round of the chip's workgroups allows).
__global__ void tile_pair_keys_kernel(uint64_t m_rows, const uint32_t *__restrict__ tincl, const uint32_t *__restrict__ hrow,
                                      const uint32_t *__restrict__ rowstart, const uint32_t *__restrict__ ploc,
                                      const uint32_t *__restrict__ wordoff, uint64_t *__restrict__ keys) {
    const uint64_t m = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= m_rows) return;
    const uint64_t t = tincl[m] - 1;
    const uint32_t r = hrow[m], p0 = rowstart[r], cnt = rowstart[r + 1] - p0, o = wordoff[m];
    for (uint32_t j = 0; j < cnt; ++j) keys[o + j] = (t << 32) | ploc[p0 + j];
}

__global__ void dict_flag_kernel(uint64_t n, const uint64_t *__restrict__ skeys, uint32_t *__restrict__ flag) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) flag[i] = (i == 0 || skeys[i] != skeys[i - 1]) ? 1u : 0u;
}

__global__ void dict_emit_kernel(uint64_t n, const uint64_t *__restrict__ skeys, const uint32_t *__restrict__ flag,
                                 const uint32_t *__restrict__ pos, uint32_t *__restrict__ dict, uint32_t *__restrict__ dict_base) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || !flag[i]) return;
    dict[pos[i]] = (uint32_t)skeys[i];
    if (i == 0 || (skeys[i] >> 32) != (skeys[i - 1] >> 32)) dict_base[skeys[i] >> 32] = pos[i];
}

__global__ void tile_hdr_kernel(uint64_t n_tiles, uint32_t dcap, uint32_t n_slots, const uint32_t *__restrict__ batch_base,
                                const uint32_t *__restrict__ nbatch, const uint32_t *__restrict__ n_one,
                                const uint32_t *__restrict__ n_two, const uint32_t *__restrict__ dict_base,
                                TileHdr *__restrict__ hdr, BuildFlags *flags) {
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n_tiles) return;
    const uint32_t db = dict_base[t], d = (t + 1 < n_tiles ? dict_base[t + 1] : n_slots) - db;
    if (d > dcap) flags->dict_overflow = 1;
    hdr[t] = TileHdr{batch_base[t], (uint16_t)nbatch[t], (uint16_t)n_one[t], db, d | (n_two[t] << 16)};
}

// one thread per (merged) row: emit its words at the padded position.  repeat (the fold, em_layout.h): a one-word row's
// pos / rem field - zero otherwise - takes the number of further identical reads the word stands for.  In a tile with a
// counted run of two-word rows (TileHdr::n_two) both words of such a row carry the row's count in that field instead of
// their positions (0 without a fold): the lane's parity says which word of the pair it is
__global__ void emit_words_kernel(uint64_t m_rows, uint32_t H, const uint32_t *__restrict__ tincl,
                                  const TileHdr *__restrict__ hdr, const uint32_t *__restrict__ dict,
                                  const uint32_t *__restrict__ hrow, const uint32_t *__restrict__ rowstart,
                                  const uint32_t *__restrict__ ploc, const uint32_t *__restrict__ pmask,
                                  const uint32_t *__restrict__ rowpad, uint32_t *__restrict__ words,
                                  const double *__restrict__ row_weight, double *__restrict__ word_weight,
                                  const uint32_t *__restrict__ row_orig, uint32_t *__restrict__ word_row,
                                  const uint32_t *__restrict__ repeat) {
    const uint64_t m = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= m_rows) return;
    const TileHdr th = hdr[tincl[m] - 1];
    const uint32_t PB = pos_bits(H);
    const uint32_t r = hrow[m], p0 = rowstart[r], cnt = rowstart[r + 1] - p0;
    const uint32_t off = rowpad[m];
    const uint64_t base = (uint64_t)th.batch_base * 64 + off;
    const uint32_t *d = dict + th.dict_base;
    for (uint32_t j = 0; j < cnt; ++j) {
        const uint32_t l = ploc[p0 + j];
        uint32_t lo = 0, hi = th.dict_count();          // lower_bound; l is present by construction
        while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            if (d[mid] < l) lo = mid + 1; else hi = mid;
        }
        uint32_t w = pmask[p0 + j] | (j << H) | ((cnt - 1 - j) << (H + PB)) | (lo << (H + 2 * PB));
        if (cnt == 2u && th.n_two() != 0u) w = pmask[p0 + j] | (lo << (H + 2 * PB));
        if (repeat && (cnt == 1u || (cnt == 2u && th.n_two() != 0u))) w |= (repeat[m] - 1u) << H;
        words[base + j] = w;
        if (word_weight) word_weight[base + j] = row_weight[m];
        if (word_row) word_row[base + j] = row_orig[r];          // resampling handle: the file row the word's weight comes from
    }
}

// The empty cells of a tile's leading one-word batches (TileHdr::n_one).  Lane g of the run holds its rows g*B .. g*B+B-1
// at batches 0 .. B-1, so without stripes only the lane of the run's last row ends early (the lanes after it are empty
// altogether and stay all-zero words: dictionary entry 0); with stripes (tile_pad_kernel) every group's last stripe can
// end in empty cells, each below a word of its own group on the same lane.  An empty cell takes the dictionary index of
// the word above it and no haplotype bit: still padding to every reader (no bit, nothing added), and a lane that walks
// down the run never meets a change of entry that is not one.  Their pos / rem field - a repeat count in these batches - is 0: the first loop
// multiplies a padding word's 4.49e307 by 1 + count, and inf times the 0.0 of a clear haplotype bit would be NaN.
// One thread per (tile, lane).
__global__ void fill_one_word_cells_kernel(uint64_t n_tiles, uint32_t H, const TileHdr *__restrict__ hdr,
                                           uint32_t *__restrict__ words) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_tiles * 64) return;
    const TileHdr th = hdr[i >> 6];
    // (the run of two-word rows, TileHdr::n_two, is laid out the same way on lane PAIRS - the two lanes of the pair that
    // ends early end at the same batch, so each of them fills its own cells exactly as a lane of the one-word run does)
    for (int run = 0; run < 2; ++run) {
        const uint32_t B = run == 0 ? th.n_one : th.n_two();
        if (B < 2) continue;
        uint32_t *w = words + ((uint64_t)th.batch_base + (run == 0 ? 0u : th.n_one)) * 64 + (i & 63u);
        // from the top: a real word has a haplotype bit, every other cell takes the index of the last real word above it
        // (none above: the lane is empty altogether - a stripe's first cell is never empty - and stays on entry 0)
        uint32_t fill = 0;
        for (uint32_t b = 0; b < B; ++b) {
            const uint32_t x = w[(uint64_t)b * 64];
            if (x & ((1u << H) - 1u)) fill = x & ~((1u << (H + 2 * pos_bits(H))) - 1u);
            else if (x != fill) w[(uint64_t)b * 64] = fill;
        }
    }
}

__global__ void iota_kernel(uint64_t n, uint32_t *__restrict__ v) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) v[i] = (uint32_t)i;
}

// destination entries of a slot: one for a locus, [header, one per member] for a locus set
__global__ void dest_count_kernel(uint64_t ns, uint32_t L, const uint32_t *__restrict__ dict, const uint32_t *__restrict__ set_ptr,
                                  uint32_t *__restrict__ cnt) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ns) return;
    const uint32_t id = dict[i];
    cnt[i] = id < L ? 1u : 1u + (set_ptr[id - L + 1] - set_ptr[id - L]);
}

// eloc / eidx: (locus, own index) of every entry; slot_dest of a locus slot = its entry (routed below), of a set slot
// = SLOT_SET | offset of its header in dest_list, dest_list[header] = number of members
__global__ void dest_emit_kernel(uint64_t ns, uint32_t L, const uint32_t *__restrict__ dict, const uint32_t *__restrict__ set_ptr,
                                 const uint32_t *__restrict__ members, const uint32_t *__restrict__ eoff,
                                 uint32_t *__restrict__ eloc, uint32_t *__restrict__ eidx, uint32_t *__restrict__ slot_dest,
                                 uint32_t *__restrict__ dest_list) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ns) return;
    const uint32_t id = dict[i], o = eoff[i];
    if (id < L) {
        eloc[o] = id;
        eidx[o] = o;
        slot_dest[i] = o;                    // provisional: the entry whose destination dest_route_kernel copies here
    } else {
        const uint32_t b = set_ptr[id - L], n = set_ptr[id - L + 1] - b;
        eloc[o] = L;                         // header
        eidx[o] = o;
        dest_list[o] = n;
        for (uint32_t j = 0; j < n; ++j) {
            eloc[o + 1 + j] = members[b + j];
            eidx[o + 1 + j] = o + 1 + j;
        }
        slot_dest[i] = SLOT_SET | o;
    }
}

// a locus slot takes its destination out of dest_list (where locus_class_kernel left the destination of every entry)
__global__ void dest_route_kernel(uint64_t ns, const uint32_t *__restrict__ dest_list, uint32_t *__restrict__ slot_dest) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ns) return;
    const uint32_t d = slot_dest[i];
    if (!(d & SLOT_SET)) slot_dest[i] = dest_list[d];
}

// Last step of the build: the dictionary and the destinations in the form the E-step kernel reads (em_layout.h) - a
// two-member set carries its members and its two destinations in place (one round trip less in the tile's prologue and
// epilogue than the general set's lists), a larger set its index.
__global__ void encode_sets_kernel(uint64_t ns, uint32_t L, const uint32_t *__restrict__ set_ptr, const uint32_t *__restrict__ members,
                                   const uint32_t *__restrict__ dest_list, uint32_t *__restrict__ dict, uint32_t *__restrict__ dict_b,
                                   uint32_t *__restrict__ slot_dest, uint32_t *__restrict__ dest_b) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ns) return;
    const uint32_t id = dict[i];
    dict_b[i] = 0;
    dest_b[i] = 0;
    if (id < L) return;
    const uint32_t k = id - L, b = set_ptr[k], n = set_ptr[k + 1] - b;
    if (n == 2) {
        const uint32_t off = slot_dest[i] & ~SLOT_SET;
        dict[i] = DICT_PAIR | members[b];
        dict_b[i] = members[b + 1];
        slot_dest[i] = SLOT_PAIR | dest_list[off + 1];      // (a destination is a row < 2^29 or SLOT_DIRECT | locus < 2^27)
        dest_b[i] = dest_list[off + 2];
    } else {
        dict[i] = DICT_SET | k;
    }
}

__global__ void slot_ptr_kernel(uint32_t L, uint64_t n_slots, const uint32_t *__restrict__ sorted_loc,
                                uint32_t *__restrict__ slot_ptr) {
    const uint32_t l = blockIdx.x * blockDim.x + threadIdx.x;
    if (l > L) return;
    uint64_t lo = 0, hi = n_slots;                   // first index with sorted_loc >= l
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        if (sorted_loc[mid] < l) lo = mid + 1; else hi = mid;
    }
    slot_ptr[l] = (uint32_t)lo;
}

__global__ void locus_class_kernel(uint32_t L, const uint32_t *__restrict__ slot_ptr, const uint32_t *__restrict__ slot_list,
                                   uint8_t *__restrict__ cls, uint32_t *__restrict__ slot_dest) {
    const uint32_t l = blockIdx.x * blockDim.x + threadIdx.x;
    if (l >= L) return;
    const uint32_t k0 = slot_ptr[l], cnt = slot_ptr[l + 1] - k0;
    cls[l] = cnt == 0 ? 0 : (cnt == 1 ? 1 : (cnt <= (uint32_t)HEAVY_SLOTS ? 2 : 3));
    // Destination of every (tile, dictionary entry) sum: straight into A for a locus that lives in one
    // tile; otherwise row k of `partials`, k = the entry's rank in the inverted index, so that the
    // slots of a locus are consecutive rows and the gather streams them without an indirection.
    // (slot_list holds entry indices, slot_dest here is the per-entry destination array: dest_list)
    if (cnt == 1) slot_dest[slot_list[k0]] = SLOT_DIRECT | l;
    else
        for (uint32_t k = k0; k < k0 + cnt; ++k) slot_dest[slot_list[k]] = k;
}

__global__ void long_rows_kernel(uint64_t n_long, uint64_t first, const uint32_t *__restrict__ srow,
                                 const uint32_t *__restrict__ rowstart, const uint32_t *__restrict__ row_orig,
                                 const double *__restrict__ count, uint64_t *__restrict__ len,
                                 double *__restrict__ weight, uint32_t *__restrict__ long_row) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_long) return;
    const uint32_t r = srow[first + i];
    len[i] = rowstart[r + 1] - rowstart[r];
    weight[i] = count ? count[row_orig[r]] : 1.0;
    if (long_row) long_row[i] = row_orig[r];
}

__global__ void long_copy_kernel(uint64_t n_long, uint64_t first, const uint32_t *__restrict__ srow,
                                 const uint32_t *__restrict__ rowstart, const uint32_t *__restrict__ ploc,
                                 const uint32_t *__restrict__ pmask, const uint64_t *__restrict__ long_ptr,
                                 uint32_t *__restrict__ long_loc, uint32_t *__restrict__ long_mask) {
    const uint64_t i = blockIdx.x;
    if (i >= n_long) return;
    const uint32_t r = srow[first + i], p0 = rowstart[r], cnt = rowstart[r + 1] - p0;
    const uint64_t o = long_ptr[i];
    for (uint32_t j = threadIdx.x; j < cnt; j += blockDim.x) {
        long_loc[o + j] = ploc[p0 + j];
        long_mask[o + j] = pmask[p0 + j];
    }
}

}  // namespace

// ---- `--report-alignment-counts` (AlignmentPropertyMatrix.py:389-459) -------------------------
constexpr uint64_t COUNT_KEY_DROPPED = ~0ull;
__global__ void __launch_bounds__(256)
count_keys_kernel(uint64_t n, uint32_t ncols, uint32_t L, uint64_t R, const uint64_t *__restrict__ col_ptr,
                  const uint32_t *__restrict__ ent_row, const int32_t *__restrict__ locus_group,
                  uint64_t *__restrict__ keys, BuildFlags *flags) {
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k - (threadIdx.x & 63) >= n) return;
    const bool live = k < n;
    const uint32_t c = entry_column(col_ptr, ncols, live ? k : n - 1, n);
    if (!live) return;
    const uint32_t h = c / L, l = c - h * L;
    const uint32_t r = ent_row[k];
    const int32_t lo = locus_group ? locus_group[l] : (int32_t)l;
    if (r >= R) flags->bad_row = 1;
    // an entry of a locus outside every group disappears from the bundled matrix
    // (AlignmentPropertyMatrix.py:155-188: the product with grp_conv_mat has no column for it); such
    // entries, like out-of-range row ids, get the all-ones key, which sorts last and is skipped below
    keys[k] = (r >= R || lo < 0) ? COUNT_KEY_DROPPED : (((uint64_t)r << 32) | ((uint64_t)(uint32_t)lo << 5) | h);
}

// per unique (row, locus', hap) entry: bump the row's entry counter; per unique (row, locus')
// pair: bump the row's locus counter
__global__ void count_rowstat_kernel(uint64_t n, const uint64_t *__restrict__ keys, uint32_t *__restrict__ nnz_row,
                                     uint32_t *__restrict__ nloc_row) {
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const uint64_t key = keys[k];
    if (key == COUNT_KEY_DROPPED) return;
    const bool new_entry = k == 0 || keys[k - 1] != key;
    const bool new_pair = k == 0 || (keys[k - 1] >> 5) != (key >> 5);
    const uint32_t r = (uint32_t)(key >> 32);
    if (new_entry) atomicAdd(&nnz_row[r], 1u);
    if (new_pair) atomicAdd(&nloc_row[r], 1u);
}

__global__ void count_accum_kernel(uint64_t n, uint32_t Lout, const uint64_t *__restrict__ keys,
                                   const uint32_t *__restrict__ nnz_row, const uint32_t *__restrict__ nloc_row,
                                   const double *__restrict__ count, double *__restrict__ aln,
                                   double *__restrict__ uniq, double *__restrict__ locus_uniq) {
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const uint64_t key = keys[k];
    if (key == COUNT_KEY_DROPPED) return;
    const bool new_entry = k == 0 || keys[k - 1] != key;
    if (!new_entry) return;
    const bool new_pair = k == 0 || (keys[k - 1] >> 5) != (key >> 5);
    const uint32_t r = (uint32_t)(key >> 32), l = (uint32_t)((key >> 5) & 0x7FFFFFFu), h = (uint32_t)(key & 31);
    const double w = count ? count[r] : 1.0;
    atomicAdd(&aln[(size_t)h * Lout + l], w);                       // integer-valued sums: exact
    if (nnz_row[r] == 1) atomicAdd(&uniq[(size_t)h * Lout + l], w);
    if (new_pair && nloc_row[r] == 1) atomicAdd(&locus_uniq[l], w);
}

struct CountsWork {
    Scratch sc;
    DevBuf<BuildFlags> d_flags;
    DevBuf<uint64_t> keys, keys2;
    DevBuf<uint32_t> nnz_row, nloc_row;
    uint64_t n = 0, rows = 0;
};
CountsWork *counts_work_new() { return new CountsWork(); }
void counts_work_free(CountsWork *w) { delete w; }

int alignment_counts_device(uint64_t R, uint32_t L, uint32_t H, uint64_t N, const uint32_t *ent_row,
                            const uint64_t *col_ptr, const double *count, const int32_t *locus_group,
                            uint32_t Lout, double *aln, double *uniq, double *locus_uniq, hipStream_t s,
                            CountsWork *work) {
    GBRS_HIP_CHECK(hipMemsetAsync(aln, 0, (size_t)H * Lout * 8, s));
    GBRS_HIP_CHECK(hipMemsetAsync(uniq, 0, (size_t)H * Lout * 8, s));
    GBRS_HIP_CHECK(hipMemsetAsync(locus_uniq, 0, (size_t)Lout * 8, s));
    if (N == 0) { GBRS_HIP_CHECK(hipStreamSynchronize(s)); return GBRS_OK; }
    CountsWork local;
    CountsWork &w = work ? *work : local;
    if (w.n != N || w.rows != R || !w.keys.p) {
        GBRS_TRY(w.d_flags.alloc(1));
        GBRS_TRY(w.keys.alloc(N)); GBRS_TRY(w.keys2.alloc(N)); GBRS_TRY(w.nnz_row.alloc(R)); GBRS_TRY(w.nloc_row.alloc(R));
        w.n = N;
        w.rows = R;
    }
    GBRS_HIP_CHECK(hipMemsetAsync(w.d_flags.p, 0, sizeof(BuildFlags), s));
    GBRS_HIP_CHECK(hipMemsetAsync(w.nnz_row.p, 0, w.nnz_row.bytes(), s));
    GBRS_HIP_CHECK(hipMemsetAsync(w.nloc_row.p, 0, w.nloc_row.bytes(), s));
    hipLaunchKernelGGL(count_keys_kernel, dim3(grid_for(N)), dim3(256), 0, s, N, H * L, L, R, col_ptr, ent_row,
                       locus_group, w.keys.p, w.d_flags.p);
    // the dropped key is all ones: within the compared bits it is larger than every real key (Lout < 2^27),
    // so dropped entries end up behind all real ones
    GBRS_TRY(sort_keys64(w.sc, w.keys.p, w.keys2.p, N, 32 + bits_for(R - 1), s));
    hipLaunchKernelGGL(count_rowstat_kernel, dim3(grid_for(N)), dim3(256), 0, s, N, w.keys2.p, w.nnz_row.p, w.nloc_row.p);
    hipLaunchKernelGGL(count_accum_kernel, dim3(grid_for(N)), dim3(256), 0, s, N, Lout, w.keys2.p, w.nnz_row.p, w.nloc_row.p,
                       count, aln, uniq, locus_uniq);
    BuildFlags hf{};
    GBRS_HIP_CHECK(hipMemcpyAsync(&hf, w.d_flags.p, sizeof(hf), hipMemcpyDeviceToHost, s));
    GBRS_HIP_CHECK(hipStreamSynchronize(s));
    GBRS_HIP_CHECK(hipGetLastError());
    if (hf.bad_row) return fail(GBRS_ERR_INVALID, "indices hold a row id >= num_rows");
    return GBRS_OK;
}

// ---- `gbrs compress` (gbrs/emase_utils.py:60-103): identical rows -> equivalence classes -------
__global__ void ec_min_row_kernel(uint64_t n, const uint32_t *__restrict__ hincl, const uint32_t *__restrict__ srow,
                                  const uint32_t *__restrict__ row_orig, const double *__restrict__ count,
                                  uint32_t *__restrict__ minrow, double *__restrict__ weight) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t g = hincl[i] - 1;
    const uint32_t r = row_orig[srow[i]];
    atomicMin(&minrow[g], r);
    atomicAdd(&weight[g], count ? count[r] : 1.0);
}

// rows without any alignment all share the empty key: one more class, at its first row's rank
__global__ void ec_empty_rows_kernel(uint64_t R, const uint32_t *__restrict__ nnz_row, const double *__restrict__ count,
                                     uint32_t *__restrict__ minrow_slot, double *__restrict__ weight_slot) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= R || nnz_row[r] != 0) return;
    atomicMin(minrow_slot, (uint32_t)r);
    atomicAdd(weight_slot, count ? count[r] : 1.0);
}

__global__ void ec_row_nnz_kernel(uint64_t n, const uint32_t *__restrict__ ent_row, uint32_t *__restrict__ nnz_row) {
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n) atomicAdd(&nnz_row[ent_row[k]], 1u);
}

__global__ void ec_rank_scatter_kernel(uint64_t n, const uint32_t *__restrict__ sorted_group, uint32_t *__restrict__ newid) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) newid[sorted_group[i]] = (uint32_t)i;
}

__global__ void ec_permute_count_kernel(uint64_t n, const uint32_t *__restrict__ newid, const double *__restrict__ w,
                                        double *__restrict__ out) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[newid[i]] = w[i];
}

// Two different rows may share a 64-bit row key.  The sort is stable in the row id, so their copies interleave
// (A B A B) and merge_flag_kernel, which compares neighbours only, starts a segment at each of them.  The four kernels
// below join the segments of equal rows inside one key run; they run only when some segment starts inside a run.
__global__ void ec_run_split_kernel(uint64_t n, const uint64_t *__restrict__ skey, const uint32_t *__restrict__ head,
                                    uint32_t *__restrict__ n_split) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i > 0 && i < n && head[i] && skey[i] == skey[i - 1]) atomicAdd(n_split, 1u);
}

__global__ void ec_segment_pos_kernel(uint64_t n, const uint32_t *__restrict__ head, const uint32_t *__restrict__ hincl,
                                      uint32_t *__restrict__ segpos) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && head[i]) segpos[hincl[i] - 1] = (uint32_t)i;
}

// alias[m] = the first segment of m's key run that holds the same row (m itself when there is none before it)
__global__ void ec_segment_alias_kernel(uint64_t n_seg, const uint32_t *__restrict__ segpos, const uint64_t *__restrict__ skey,
                                        const uint32_t *__restrict__ srow, const uint32_t *__restrict__ rowstart,
                                        const uint32_t *__restrict__ ploc, const uint32_t *__restrict__ pmask,
                                        uint32_t *__restrict__ alias, uint32_t *__restrict__ keep) {
    const uint64_t m = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= n_seg) return;
    const uint32_t i = segpos[m], rb = srow[i];
    const uint64_t k = skey[i];
    uint32_t a = (uint32_t)m;
    for (uint64_t m2 = m; m2-- > 0;) {
        const uint32_t j = segpos[m2];
        if (skey[j] != k) break;
        const uint32_t ra = srow[j];
        if (!same_loci(rowstart, ploc, ra, rb)) continue;
        const uint32_t pa = rowstart[ra], pb = rowstart[rb], cnt = rowstart[ra + 1] - pa;
        bool eq = true;
        for (uint32_t j2 = 0; j2 < cnt; ++j2) eq &= pmask[pa + j2] == pmask[pb + j2];
        if (eq) a = (uint32_t)m2;
    }
    alias[m] = a;
    keep[m] = a == (uint32_t)m;
}

// every sorted row gets the ordinal of its kept segment; a joined segment's first row stops being a head
__global__ void ec_regroup_kernel(uint64_t n, const uint32_t *__restrict__ alias, const uint32_t *__restrict__ kidx,
                                  uint32_t *__restrict__ head, uint32_t *__restrict__ hincl) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t m = hincl[i] - 1, a = alias[m];
    if (a != m) head[i] = 0;
    hincl[i] = kidx[a] + 1;
}

__global__ void ec_count_entries_kernel(uint64_t n_short, const uint32_t *__restrict__ head, const uint32_t *__restrict__ srow,
                                        const uint32_t *__restrict__ rowstart, const uint32_t *__restrict__ pmask,
                                        uint32_t *__restrict__ nent) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_short) return;
    uint32_t c = 0;
    if (head[i]) {
        const uint32_t r = srow[i];
        for (uint32_t p = rowstart[r]; p < rowstart[r + 1]; ++p) c += __popc(pmask[p]);
    }
    nent[i] = c;
}

__global__ void ec_emit_entries_kernel(uint64_t n_short, const uint32_t *__restrict__ head, const uint32_t *__restrict__ hincl,
                                       const uint32_t *__restrict__ srow, const uint32_t *__restrict__ rowstart,
                                       const uint32_t *__restrict__ ploc, const uint32_t *__restrict__ pmask,
                                       const uint32_t *__restrict__ eoff, const uint32_t *__restrict__ newid,
                                       uint64_t *__restrict__ keys) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_short || !head[i]) return;
    const uint32_t r = srow[i];
    const uint64_t id = newid[hincl[i] - 1];
    uint32_t o = eoff[i];
    for (uint32_t p = rowstart[r]; p < rowstart[r + 1]; ++p) {
        uint32_t m = pmask[p];
        while (m) {
            const uint32_t h = __ffs(m) - 1;
            m &= m - 1;
            keys[o++] = ((uint64_t)h << 59) | ((uint64_t)ploc[p] << 32) | id;     // sort by (hap, locus, class)
        }
    }
}

__global__ void ec_split_kernel(uint64_t n, const uint64_t *__restrict__ keys, uint32_t *__restrict__ indices) {
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n) indices[k] = (uint32_t)(keys[k] & 0xFFFFFFFFu);
}

__global__ void ec_indptr_kernel(uint32_t L, uint32_t H, uint64_t n, const uint64_t *__restrict__ keys,
                                 uint64_t *__restrict__ colptr) {
    const uint64_t c = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;   // column id h*L + l, plus the end
    if (c > (uint64_t)H * L) return;
    const uint64_t h = c / L, l = c - h * L;
    const uint64_t target = c == (uint64_t)H * L ? ~0ull : ((h << 59) | (l << 32));
    uint64_t lo = 0, hi = n;
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        if (keys[mid] < target) lo = mid + 1; else hi = mid;
    }
    colptr[c] = lo;
}

// ---- what compress_device and build_tile_layout share -------------------------------------------------------------------
namespace {

// exclusive scan of n counts; `total` is their sum, which `close` also writes behind the offsets (out[n])
template <typename T>
int scan_total(Scratch &sc, const T *in, T *out, size_t n, T &total, hipStream_t s, bool close = false) {
    GBRS_TRY(exclusive_scan(sc, in, out, n, s));
    GBRS_TRY(fetch_last_plus(out, in, n, total, s));
    if (close) GBRS_HIP_CHECK(hipMemcpyAsync(out + n, &total, sizeof(T), hipMemcpyHostToDevice, s));
    return GBRS_OK;
}

// inclusive scan of n > 0 head flags; `total` is the number of heads
int scan_heads(Scratch &sc, const uint32_t *head, uint32_t *incl, size_t n, uint32_t &total, hipStream_t s) {
    GBRS_TRY(inclusive_scan(sc, head, incl, n, s));
    GBRS_HIP_CHECK(hipMemcpyAsync(&total, incl + n - 1, 4, hipMemcpyDeviceToHost, s));
    GBRS_HIP_CHECK(hipStreamSynchronize(s));
    return GBRS_OK;
}

int running_max(Scratch &sc, const uint32_t *in, uint32_t *out, size_t n, hipStream_t s) {
    size_t bytes = 0;
    GBRS_PRIM(rocprim::inclusive_scan(nullptr, bytes, in, out, n, rocprim::maximum<uint32_t>(), s));
    GBRS_TRY(sc.reserve(bytes));
    GBRS_PRIM(rocprim::inclusive_scan(sc.buf.p, bytes, in, out, n, rocprim::maximum<uint32_t>(), s));
    return GBRS_OK;
}

// the stream, the scan / sort scratch and the flags the kernels of a build raise
struct Build {
    hipStream_t s;
    StageTimer *stg;             // null: no checkpoints (compress_device)
    Scratch sc;
    DevBuf<BuildFlags> d_flags;
    BuildFlags hf{};
    Build(hipStream_t stream, StageTimer *timer) : s(stream), stg(timer) {}
    int init() {
        GBRS_TRY(d_flags.alloc(1));
        GBRS_HIP_CHECK(hipMemsetAsync(d_flags.p, 0, sizeof(BuildFlags), s));
        return GBRS_OK;
    }
    int read_flags() {
        GBRS_HIP_CHECK(hipMemcpyAsync(&hf, d_flags.p, sizeof(hf), hipMemcpyDeviceToHost, s));
        GBRS_HIP_CHECK(hipStreamSynchronize(s));
        return GBRS_OK;
    }
    void mark(const char *stage) { if (stg) stg->mark(stage); }
};

// the rows with at least one alignment as (locus, haplotype mask) pairs: pairs rowstart[r] .. rowstart[r + 1] of row r,
// which is row row_orig[r] of the input
struct RowPairs {
    DevBuf<uint32_t> rowstart, row_orig, ploc, pmask;
    uint64_t P = 0, R1 = 0;
    void release() { rowstart.release(); row_orig.release(); ploc.release(); pmask.release(); }
};

// entries -> sorted (row, locus, hap) keys -> pairs -> rows (N > 0).  The keys carry the row above bit row_shift.
// view > 1: L and H are those of the half-locus view, the CSC columns those of the caller's L / view loci with H * view
// haplotypes.
int build_row_pairs(Build &b, RowPairs &rp, uint64_t R, uint32_t L, uint32_t H, uint64_t N, const uint32_t *ent_row,
                    const uint64_t *col_ptr, unsigned row_shift, uint32_t view = 1) {
    hipStream_t s = b.s;
    // 1. entries -> sorted (row, locus, hap) keys
    DevBuf<uint64_t> keys, keys2;
    GBRS_TRY(keys.alloc(N)); GBRS_TRY(keys2.alloc(N));
    b.mark("1a key buffers");
    hipLaunchKernelGGL(make_keys_kernel, dim3(grid_for(N, 4 * KEY_SPAN)), dim3(256), 0, s, N, H * L, L / view, R, row_shift,
                       col_ptr, ent_row, keys.p, b.d_flags.p, view > 1 ? H : 0u);
    b.mark("1b make keys");
    GBRS_TRY(sort_keys64(b.sc, keys.p, keys2.p, N, row_shift + bits_for(R - 1), s));
    b.mark("1c sort entries");
    keys.release();
    b.mark("1d release");
    // 2. pairs
    DevBuf<uint32_t> pflag, pidx;
    GBRS_TRY(pflag.alloc(N)); GBRS_TRY(pidx.alloc(N));
    b.mark("2a alloc flags");
    hipLaunchKernelGGL(pair_flag_kernel, dim3(grid_for(N)), dim3(256), 0, s, N, keys2.p, pflag.p, b.d_flags.p);
    b.mark("2b pair flags");
    GBRS_TRY(exclusive_scan(b.sc, pflag.p, pidx.p, N, s));
    b.mark("2c scan");
    uint32_t P32 = 0;
    GBRS_TRY(fetch_last_plus(pidx.p, pflag.p, N, P32, s));
    GBRS_TRY(b.read_flags());
    b.mark("2d fetch");
    if (b.hf.bad_row) return fail(GBRS_ERR_INVALID, "indices hold a row id >= num_rows");
    if (b.hf.duplicate) return fail(GBRS_ERR_INVALID, "duplicate (row, locus, haplotype) entry: the CSC arrays must be canonical");
    rp.P = P32;
    DevBuf<uint32_t> prow;
    GBRS_TRY(prow.alloc(rp.P)); GBRS_TRY(rp.ploc.alloc(rp.P)); GBRS_TRY(rp.pmask.alloc(rp.P));
    hipLaunchKernelGGL(emit_pairs_kernel, dim3(grid_for(N)), dim3(256), 0, s, N, keys2.p, pflag.p, pidx.p, row_shift,
                       prow.p, rp.ploc.p, rp.pmask.p);
    GBRS_HIP_CHECK(hipStreamSynchronize(s));
    b.mark("2e emit pairs");
    keys2.release(); pflag.release(); pidx.release();
    b.mark("2 pairs (release)");
    // 3. rows
    DevBuf<uint32_t> rflag, ridx;
    GBRS_TRY(rflag.alloc(rp.P)); GBRS_TRY(ridx.alloc(rp.P));
    hipLaunchKernelGGL(row_flag_kernel, dim3(grid_for(rp.P)), dim3(256), 0, s, rp.P, prow.p, rflag.p);
    uint32_t R32 = 0;
    GBRS_TRY(scan_total(b.sc, rflag.p, ridx.p, rp.P, R32, s));
    rp.R1 = R32;
    GBRS_TRY(rp.rowstart.alloc((size_t)rp.R1 + 1)); GBRS_TRY(rp.row_orig.alloc(rp.R1));
    hipLaunchKernelGGL(row_start_kernel, dim3(grid_for(rp.P)), dim3(256), 0, s, rp.P, rp.R1, rflag.p, ridx.p, prow.p,
                       rp.rowstart.p, rp.row_orig.p);
    GBRS_HIP_CHECK(hipStreamSynchronize(s));
    return GBRS_OK;        // (rflag, ridx and prow go here)
}

}  // namespace

int compress_device(CompressResult &out, uint64_t R, uint32_t L, uint32_t H, uint64_t N, const uint32_t *ent_row,
                    const uint64_t *col_ptr, const double *count, hipStream_t s) {
    if (H > 16 || N >= 0xFFFFFFFFull || L >= (1u << 27))
        return fail(GBRS_ERR_INVALID, "compress needs H <= 16, N < 2^32 entries and L < 2^27 loci");
    Build b(s, nullptr);
    GBRS_TRY(b.init());
    Scratch &sc = b.sc;
    out.num_ecs = 0;
    out.n_entries = 0;
    GBRS_TRY(out.col_ptr.alloc((size_t)H * L + 1));
    GBRS_HIP_CHECK(hipMemsetAsync(out.col_ptr.p, 0, out.col_ptr.bytes(), s));
    // rows without alignments
    DevBuf<uint32_t> nnz_row;
    GBRS_TRY(nnz_row.alloc(R));
    GBRS_HIP_CHECK(hipMemsetAsync(nnz_row.p, 0, nnz_row.bytes(), s));
    if (N) hipLaunchKernelGGL(ec_row_nnz_kernel, dim3(grid_for(N)), dim3(256), 0, s, N, ent_row, nnz_row.p);
    uint64_t R1 = 0, M = 0;
    RowPairs rp;
    DevBuf<uint32_t> &ploc = rp.ploc, &pmask = rp.pmask, &rowstart = rp.rowstart, &row_orig = rp.row_orig;
    DevBuf<uint32_t> srow, head, hincl;
    if (N) {
        GBRS_TRY(build_row_pairs(b, rp, R, L, H, N, ent_row, col_ptr, 32u));
        R1 = rp.R1;
        DevBuf<uint64_t> rkey, skey;
        DevBuf<uint32_t> ident;
        GBRS_TRY(rkey.alloc(R1)); GBRS_TRY(skey.alloc(R1)); GBRS_TRY(ident.alloc(R1)); GBRS_TRY(srow.alloc(R1));
        const unsigned lbits = bits_for(L - 1);
        hipLaunchKernelGGL(row_key_kernel, dim3(grid_for(R1)), dim3(256), 0, s, R1, 0xFFFFFFFFu, lbits > 24 ? lbits - 24 : 0u,
                           rowstart.p, ploc.p, pmask.p, rkey.p, ident.p, b.d_flags.p);
        GBRS_TRY(sort_pairs<uint64_t>(sc, rkey.p, skey.p, ident.p, srow.p, R1, 64, s));
        GBRS_TRY(head.alloc(R1)); GBRS_TRY(hincl.alloc(R1));
        hipLaunchKernelGGL(merge_flag_kernel, dim3(grid_for(R1)), dim3(256), 0, s, R1, 1, skey.p, srow.p, rowstart.p, ploc.p,
                           pmask.p, head.p);
        GBRS_TRY(inclusive_scan(sc, head.p, hincl.p, R1, s));
        DevBuf<uint32_t> d_split;
        GBRS_TRY(d_split.alloc(1));
        GBRS_HIP_CHECK(hipMemsetAsync(d_split.p, 0, 4, s));
        hipLaunchKernelGGL(ec_run_split_kernel, dim3(grid_for(R1)), dim3(256), 0, s, R1, skey.p, head.p, d_split.p);
        uint32_t m32 = 0, n_split = 0;
        GBRS_HIP_CHECK(hipMemcpyAsync(&m32, hincl.p + R1 - 1, 4, hipMemcpyDeviceToHost, s));
        GBRS_HIP_CHECK(hipMemcpyAsync(&n_split, d_split.p, 4, hipMemcpyDeviceToHost, s));
        GBRS_HIP_CHECK(hipStreamSynchronize(s));
        M = m32;
        if (n_split) {   // different rows under one key: join the segments that hold the same row
            DevBuf<uint32_t> segpos, alias, keep, kidx;
            GBRS_TRY(segpos.alloc(M)); GBRS_TRY(alias.alloc(M)); GBRS_TRY(keep.alloc(M)); GBRS_TRY(kidx.alloc(M));
            hipLaunchKernelGGL(ec_segment_pos_kernel, dim3(grid_for(R1)), dim3(256), 0, s, R1, head.p, hincl.p, segpos.p);
            hipLaunchKernelGGL(ec_segment_alias_kernel, dim3(grid_for(M)), dim3(256), 0, s, M, segpos.p, skey.p, srow.p, rowstart.p,
                               ploc.p, pmask.p, alias.p, keep.p);
            GBRS_TRY(scan_total(sc, keep.p, kidx.p, M, m32, s));
            hipLaunchKernelGGL(ec_regroup_kernel, dim3(grid_for(R1)), dim3(256), 0, s, R1, alias.p, kidx.p, head.p, hincl.p);
            GBRS_HIP_CHECK(hipStreamSynchronize(s));
            M = m32;
        }
    }
    // classes: M from rows with alignments (+1 for the empty key if any row is empty)
    DevBuf<uint32_t> minrow;
    DevBuf<double> weight;
    GBRS_TRY(minrow.alloc(M + 1));
    GBRS_TRY(weight.alloc(M + 1));
    GBRS_HIP_CHECK(hipMemsetAsync(minrow.p, 0xFF, minrow.bytes(), s));
    GBRS_HIP_CHECK(hipMemsetAsync(weight.p, 0, weight.bytes(), s));
    if (R1) hipLaunchKernelGGL(ec_min_row_kernel, dim3(grid_for(R1)), dim3(256), 0, s, R1, hincl.p, srow.p, row_orig.p, count,
                               minrow.p, weight.p);
    hipLaunchKernelGGL(ec_empty_rows_kernel, dim3(grid_for(R)), dim3(256), 0, s, R, nnz_row.p, count, minrow.p + M,
                       weight.p + M);
    uint32_t empty_first = 0xFFFFFFFFu;
    GBRS_HIP_CHECK(hipMemcpyAsync(&empty_first, minrow.p + M, 4, hipMemcpyDeviceToHost, s));
    GBRS_HIP_CHECK(hipStreamSynchronize(s));
    const uint64_t G = M + (empty_first != 0xFFFFFFFFu ? 1 : 0);
    out.num_ecs = G;
    if (G == 0) return GBRS_OK;
    // first-seen order (dict insertion order of the reference, :77, :95): rank classes by first row
    DevBuf<uint32_t> gid, gsorted, msorted, newid;
    GBRS_TRY(gid.alloc(G)); GBRS_TRY(gsorted.alloc(G)); GBRS_TRY(msorted.alloc(G)); GBRS_TRY(newid.alloc(G));
    hipLaunchKernelGGL(iota_kernel, dim3(grid_for(G)), dim3(256), 0, s, G, gid.p);
    GBRS_TRY(sort_pairs<uint32_t>(sc, minrow.p, msorted.p, gid.p, gsorted.p, G, 32, s));
    hipLaunchKernelGGL(ec_rank_scatter_kernel, dim3(grid_for(G)), dim3(256), 0, s, G, gsorted.p, newid.p);
    GBRS_TRY(out.count.alloc(G));
    {   // counts in the new order
        DevBuf<double> tmpw;
        GBRS_TRY(tmpw.alloc(G));
        GBRS_HIP_CHECK(hipMemcpyAsync(tmpw.p, weight.p, G * 8, hipMemcpyDeviceToDevice, s));
        // out.count[newid[g]] = weight[g]
        hipLaunchKernelGGL(ec_permute_count_kernel, dim3(grid_for(G)), dim3(256), 0, s, G, newid.p, tmpw.p, out.count.p);
        GBRS_HIP_CHECK(hipStreamSynchronize(s));
    }
    if (R1 == 0) return GBRS_OK;
    // entries of the representative rows, relabelled and ordered by (hap, locus, class)
    DevBuf<uint32_t> nent, eoff;
    GBRS_TRY(nent.alloc(R1)); GBRS_TRY(eoff.alloc(R1));
    hipLaunchKernelGGL(ec_count_entries_kernel, dim3(grid_for(R1)), dim3(256), 0, s, R1, head.p, srow.p, rowstart.p, pmask.p,
                       nent.p);
    uint32_t E32 = 0;
    GBRS_TRY(scan_total(sc, nent.p, eoff.p, R1, E32, s));
    const uint64_t E = E32;
    out.n_entries = E;
    DevBuf<uint64_t> ekeys, ekeys2;
    GBRS_TRY(ekeys.alloc(E)); GBRS_TRY(ekeys2.alloc(E));
    hipLaunchKernelGGL(ec_emit_entries_kernel, dim3(grid_for(R1)), dim3(256), 0, s, R1, head.p, hincl.p, srow.p, rowstart.p,
                       ploc.p, pmask.p, eoff.p, newid.p, ekeys.p);
    GBRS_TRY(sort_keys64(sc, ekeys.p, ekeys2.p, E, 64, s));
    GBRS_TRY(out.indices.alloc(E));
    hipLaunchKernelGGL(ec_split_kernel, dim3(grid_for(E)), dim3(256), 0, s, E, ekeys2.p, out.indices.p);
    hipLaunchKernelGGL(ec_indptr_kernel, dim3(grid_for((uint64_t)H * L + 1)), dim3(256), 0, s, L, H, E, ekeys2.p,
                       out.col_ptr.p);
    GBRS_HIP_CHECK(hipStreamSynchronize(s));
    GBRS_HIP_CHECK(hipGetLastError());
    return GBRS_OK;
}

// ---- the stages of build_tile_layout ---------------------------------------------------------------------------------------
namespace {

// The tail of both forms of the locus sets.  V sets of set_len[v] member loci each have been found: their member lists
// (`members` launches the kernel that fills out.set_members), the rows' new lengths (`row_len`, into newlen), the rows
// rewritten with one pair per set (`rewrite`, from rowstart2 into ploc2 / pmask2), and - when `use(P2)` says that the P2
// pairs left are worth it - the new rows in place of the old ones.
template <typename Members, typename RowLen, typename Rewrite, typename Use>
int finish_locus_sets(Build &b, TileLayout &out, RowPairs &rp, uint32_t V, const uint32_t *set_len, Members members,
                      RowLen row_len, Rewrite rewrite, Use use) {
    hipStream_t s = b.s;
    const uint64_t R1 = rp.R1;
    GBRS_TRY(out.set_ptr.alloc((size_t)V + 1));
    uint32_t n_members = 0;
    GBRS_TRY(scan_total(b.sc, set_len, out.set_ptr.p, V, n_members, s, true));
    GBRS_TRY(out.set_members.alloc(n_members));
    members();
    DevBuf<uint32_t> newlen, rowstart2, ploc2, pmask2;
    GBRS_TRY(newlen.alloc(R1)); GBRS_TRY(rowstart2.alloc((size_t)R1 + 1));
    row_len(newlen.p);
    uint32_t P2 = 0;
    GBRS_TRY(scan_total(b.sc, newlen.p, rowstart2.p, R1, P2, s, true));
    GBRS_TRY(ploc2.alloc(P2)); GBRS_TRY(pmask2.alloc(P2));
    rewrite(rowstart2.p, ploc2.p, pmask2.p);
    GBRS_HIP_CHECK(hipStreamSynchronize(s));
    GBRS_HIP_CHECK(hipGetLastError());
    if (use(P2)) {
        rp.rowstart.swap(rowstart2); rp.ploc.swap(ploc2); rp.pmask.swap(pmask2);
        out.n_sets = V;            // ids of the rows' pairs, the sort keys and the dictionaries are loci + sets from here on
        out.n_pairs = P2;
    } else {
        out.set_ptr.release();
        out.set_members.release();
    }
    return GBRS_OK;
}

// 3b. locus sets, first form (round 3): a row whose pairs ALL carry one mask becomes one pair on the id of its locus set
// (em_layout.h), every distinct set kept.  Round 4's step 3c below finds the same sets (a whole row is a row with one mask
// group) and keeps the frequent ones only, which is what the samples want (C2: all 98,725 sets 0.0901 ms per iteration,
// the 17-42 k sets carried by >= 128 / 32 reads 0.0857); this form stays reachable with GBRS_TUNING_LOCUS_SETS=1.
int whole_row_sets(Build &b, TileLayout &out, RowPairs &rp, const EmPlan &plan) {
    hipStream_t s = b.s;
    Scratch &sc = b.sc;
    const uint64_t R1 = rp.R1, P = rp.P;
    const uint32_t L_in = plan.tL;
    const uint32_t *rowstart = rp.rowstart.p, *ploc = rp.ploc.p, *pmask = rp.pmask.p;
    DevBuf<uint64_t> key, ckey, skey2;
    DevBuf<uint32_t> flag, cidx, crow, srow2;
    GBRS_TRY(key.alloc(R1)); GBRS_TRY(flag.alloc(R1)); GBRS_TRY(cidx.alloc(R1));
    hipLaunchKernelGGL(set_candidate_kernel, dim3(grid_for(R1)), dim3(256), 0, s, R1, rowstart, ploc, pmask, key.p, flag.p);
    uint32_t C = 0;
    GBRS_TRY(scan_total(sc, flag.p, cidx.p, R1, C, s));
    if (C == 0) return GBRS_OK;
    GBRS_TRY(ckey.alloc(C)); GBRS_TRY(skey2.alloc(C)); GBRS_TRY(crow.alloc(C)); GBRS_TRY(srow2.alloc(C));
    hipLaunchKernelGGL(set_compact_kernel, dim3(grid_for(R1)), dim3(256), 0, s, R1, flag.p, cidx.p, key.p, ckey.p, crow.p);
    GBRS_TRY(sort_pairs<uint64_t>(sc, ckey.p, skey2.p, crow.p, srow2.p, C, 64, s));
    key.release(); ckey.release(); crow.release();
    DevBuf<uint32_t> head2, hincl2, set_of_row;
    GBRS_TRY(head2.alloc(C)); GBRS_TRY(hincl2.alloc(C)); GBRS_TRY(set_of_row.alloc(R1));
    hipLaunchKernelGGL(set_head_kernel, dim3(grid_for(C)), dim3(256), 0, s, (uint64_t)C, skey2.p, srow2.p, rowstart, ploc, head2.p);
    uint32_t V = 0;
    GBRS_TRY(scan_heads(sc, head2.p, hincl2.p, C, V, s));
    // (ids of loci and sets share the 27 bits of a row key: a sample with that many distinct sets keeps its plain rows)
    if ((uint64_t)L_in + V >= (1u << 27)) return GBRS_OK;
    DevBuf<uint32_t> set_len, set_rep;
    GBRS_TRY(set_len.alloc(V)); GBRS_TRY(set_rep.alloc(V));
    GBRS_HIP_CHECK(hipMemsetAsync(set_of_row.p, 0xFF, set_of_row.bytes(), s));
    hipLaunchKernelGGL(set_assign_kernel, dim3(grid_for(C)), dim3(256), 0, s, (uint64_t)C, head2.p, hincl2.p, srow2.p, rowstart,
                       set_of_row.p, set_len.p, set_rep.p);
    return finish_locus_sets(
        b, out, rp, V, set_len.p,
        [&] { hipLaunchKernelGGL(set_members_kernel, dim3(grid_for(V)), dim3(256), 0, s, V, out.set_ptr.p, set_rep.p, rowstart, ploc,
                                 out.set_members.p); },
        [&](uint32_t *newlen) { hipLaunchKernelGGL(set_row_len_kernel, dim3(grid_for(R1)), dim3(256), 0, s, R1, rowstart,
                                                   set_of_row.p, newlen); },
        [&](const uint32_t *rowstart2, uint32_t *ploc2, uint32_t *pmask2) {
            hipLaunchKernelGGL(set_rewrite_kernel, dim3(grid_for(R1)), dim3(256), 0, s, R1, L_in, rowstart, set_of_row.p, rowstart2,
                               ploc, pmask, ploc2, pmask2); },
        [&](uint32_t P2) { return em_use_whole_row_sets(plan, P, P2, L_in, V); });
}

// 3c. locus sets per mask group, when the rows are no whole-row sets (reads over several isoforms with differing masks):
// the loci of a row that share a mask become one pair on a set id, for the sets that enough rows carry
int mask_group_sets(Build &b, TileLayout &out, RowPairs &rp, const EmPlan &plan) {
    hipStream_t s = b.s;
    Scratch &sc = b.sc;
    const uint64_t R1 = rp.R1, P = rp.P;
    const uint32_t L_in = plan.tL;
    const uint32_t *rowstart = rp.rowstart.p, *ploc = rp.ploc.p, *pmask = rp.pmask.p;
    // rows a set must be carried by.  Iteration time, one box each: multi-isoform sample (2.35 words per read, no sets 0.1970 ms):
    // 64 rows (39 k sets) 0.199, 128 (21 k) 0.188, 160: 0.186, 192 (13.8 k) 0.184, 256 (10 k) 0.183, 384 / 512: 0.184;
    // C2 (whole-row sets, all 98.7 k of them 0.0901 ms): 32 rows (42.5 k) 0.0858, 128 (17 k) 0.0857, 512 (4.3 k) 0.0881
    uint32_t min_rows = plan.set_min_rows;
    DevBuf<uint32_t> gloc, gmask, nseg, segoff;
    GBRS_TRY(gloc.alloc(P)); GBRS_TRY(gmask.alloc(P)); GBRS_TRY(nseg.alloc(R1)); GBRS_TRY(segoff.alloc((size_t)R1 + 1));
    hipLaunchKernelGGL(group_sort_kernel, dim3(grid_for(R1)), dim3(256), 0, s, R1, rowstart, ploc, pmask, gloc.p, gmask.p, nseg.p);
    uint32_t S = 0;
    GBRS_TRY(scan_total(sc, nseg.p, segoff.p, R1, S, s, true));
    DevBuf<uint32_t> seg_begin, seg_len, cand, cidx;
    DevBuf<uint64_t> key;
    GBRS_TRY(seg_begin.alloc(S)); GBRS_TRY(seg_len.alloc(S)); GBRS_TRY(cand.alloc(S)); GBRS_TRY(cidx.alloc(S));
    GBRS_TRY(key.alloc(S));
    hipLaunchKernelGGL(group_segments_kernel, dim3(grid_for(R1)), dim3(256), 0, s, R1, rowstart, gloc.p, gmask.p, segoff.p,
                       seg_begin.p, seg_len.p, key.p, cand.p);
    uint32_t C = 0;
    GBRS_TRY(scan_total(sc, cand.p, cidx.p, S, C, s));
    if (C == 0 || S >= P) return GBRS_OK;
    DevBuf<uint64_t> ckey, skey2;
    DevBuf<uint32_t> cseg, sseg, head2, hincl2;
    GBRS_TRY(ckey.alloc(C)); GBRS_TRY(skey2.alloc(C)); GBRS_TRY(cseg.alloc(C)); GBRS_TRY(sseg.alloc(C));
    hipLaunchKernelGGL(group_compact_kernel, dim3(grid_for(S)), dim3(256), 0, s, (uint64_t)S, cand.p, cidx.p, key.p, ckey.p, cseg.p);
    GBRS_TRY(sort_pairs<uint64_t>(sc, ckey.p, skey2.p, cseg.p, sseg.p, C, 64, s));
    key.release(); ckey.release(); cseg.release(); cand.release(); cidx.release();
    GBRS_TRY(head2.alloc(C)); GBRS_TRY(hincl2.alloc(C));
    hipLaunchKernelGGL(group_head_kernel, dim3(grid_for(C)), dim3(256), 0, s, (uint64_t)C, skey2.p, sseg.p, seg_begin.p, seg_len.p,
                       gloc.p, head2.p);
    uint32_t Vp = 0;
    GBRS_TRY(scan_heads(sc, head2.p, hincl2.p, C, Vp, s));
    DevBuf<uint32_t> cnt, rep, keep, newid;
    GBRS_TRY(cnt.alloc(Vp)); GBRS_TRY(rep.alloc(Vp)); GBRS_TRY(keep.alloc(Vp)); GBRS_TRY(newid.alloc(Vp));
    GBRS_HIP_CHECK(hipMemsetAsync(cnt.p, 0, cnt.bytes(), s));
    hipLaunchKernelGGL(group_count_kernel, dim3(grid_for(C)), dim3(256), 0, s, (uint64_t)C, head2.p, hincl2.p, sseg.p, cnt.p, rep.p);
    // the frequent sets only, and no more of them than half the loci: the threshold doubles until they fit
    uint32_t V = 0;
    for (int round = 0; round < 24; ++round) {
        hipLaunchKernelGGL(group_keep_kernel, dim3(grid_for(Vp)), dim3(256), 0, s, Vp, min_rows, cnt.p, keep.p);
        GBRS_TRY(scan_total(sc, keep.p, newid.p, Vp, V, s));
        if (em_group_sets_fit(plan, V, L_in)) break;
        min_rows *= 2;
    }
    if (V == 0 || (uint64_t)L_in + V >= (1u << 27)) return GBRS_OK;
    DevBuf<uint32_t> set_of_seg, set_len, set_rep;
    GBRS_TRY(set_of_seg.alloc(S)); GBRS_TRY(set_len.alloc(V)); GBRS_TRY(set_rep.alloc(V));
    GBRS_HIP_CHECK(hipMemsetAsync(set_of_seg.p, 0xFF, set_of_seg.bytes(), s));
    hipLaunchKernelGGL(group_assign_kernel, dim3(grid_for(C)), dim3(256), 0, s, (uint64_t)C, hincl2.p, sseg.p, keep.p, newid.p, rep.p,
                       seg_len.p, set_of_seg.p, set_len.p, set_rep.p);
    return finish_locus_sets(
        b, out, rp, V, set_len.p,
        [&] { hipLaunchKernelGGL(group_members_kernel, dim3(grid_for(V)), dim3(256), 0, s, V, out.set_ptr.p, set_rep.p, seg_begin.p,
                                 gloc.p, out.set_members.p); },
        [&](uint32_t *newlen) { hipLaunchKernelGGL(group_row_len_kernel, dim3(grid_for(R1)), dim3(256), 0, s, R1, segoff.p, seg_len.p,
                                                   set_of_seg.p, newlen); },
        [&](const uint32_t *rowstart2, uint32_t *ploc2, uint32_t *pmask2) {
            hipLaunchKernelGGL(group_rewrite_kernel, dim3(grid_for(R1)), dim3(256), 0, s, R1, L_in, segoff.p, seg_begin.p, seg_len.p,
                               set_of_seg.p, rowstart2, gloc.p, gmask.p, ploc2, pmask2); },
        [&](uint32_t P2) { return em_use_group_sets(plan, P, P2); });
}

// the rows in the order of step 4: the n_short rows of the tiles first, then the n_long rows that keep their pair form
struct SortedRows {
    DevBuf<uint64_t> skey;       // (step 5 only)
    DevBuf<uint32_t> srow;
    uint64_t n_long = 0, n_short = 0;
};

// 4. order rows so that similar rows are adjacent.  L: loci + locus sets
int order_rows(Build &b, TileLayout &out, const RowPairs &rp, SortedRows &rows, uint32_t L, uint32_t H) {
    hipStream_t s = b.s;
    const uint64_t R1 = rp.R1;
    DevBuf<uint64_t> rkey;
    DevBuf<uint32_t> ident;
    GBRS_TRY(rkey.alloc(R1)); GBRS_TRY(rows.skey.alloc(R1)); GBRS_TRY(ident.alloc(R1)); GBRS_TRY(rows.srow.alloc(R1));
    const unsigned lbits = bits_for(L - 1);
    hipLaunchKernelGGL(row_key_kernel, dim3(grid_for(R1)), dim3(256), 0, s, R1, (uint32_t)max_row_words(H),
                       lbits > 24 ? lbits - 24 : 0u, rp.rowstart.p, rp.ploc.p, rp.pmask.p, rkey.p, ident.p, b.d_flags.p);
    GBRS_TRY(sort_pairs<uint64_t>(b.sc, rkey.p, rows.skey.p, ident.p, rows.srow.p, R1, 64, s));
    GBRS_TRY(b.read_flags());
    rows.n_long = b.hf.n_long;
    rows.n_short = R1 - rows.n_long;
    out.n_long = rows.n_long;
    return GBRS_OK;
}

// the short rows of the layout: row hrow[i] of the pairs, standing for 1 + repeat[i] reads where the layout folds
struct LayoutRows {
    DevBuf<uint32_t> hrow, repeat;
    uint64_t M = 0;
    bool fold = false;
    void release() { hrow.release(); repeat.release(); }
};

// 5. optional merge of identical adjacent rows + weights - or the fold of identical one-word reads (em_layout.h): the
// reads of one (dictionary entry, mask) class that the sort left next to each other keep one row with a repeat count,
// cut every FOLD_CAP rows.  The fold exists where the E-step kernels read the count: the leading one-word batches of the
// stream order's unweighted tiles (TileHdr::n_one) of the haplotype counts with a kernel instance of their own.  Reads
// of exactly two words fold the same way (fold_mode 3): their run of a tile follows its one-word batches on lane pairs
// (TileHdr::n_two), where the lane's parity stands for a word's position and both words carry the row's count.
// Both folds are tried first, then the one-word fold alone, then one row per read (em_plan.h: em_take_fold).
int merge_rows(Build &b, TileLayout &out, const RowPairs &rp, SortedRows &rows, LayoutRows &lr, const double *count,
               const EmPlan &plan) {
    hipStream_t s = b.s;
    const uint64_t n_short = rows.n_short;
    const uint32_t FOLD_CAP = 1u << (2 * pos_bits((int)plan.tH));
    const uint32_t *srow = rows.srow.p, *rowstart = rp.rowstart.p;
    bool fold = plan.fold;
    int fold_mode = plan.fold_mode;          // merge_flag_kernel's mode: 3 both folds, 2 one-word
    lr.M = n_short;
    if (n_short) {
        DevBuf<unsigned long long> two_total;
        DevBuf<uint32_t> head, hincl;
        GBRS_TRY(head.alloc(n_short)); GBRS_TRY(hincl.alloc(n_short));
        uint32_t m32 = 0;
        for (;;) {
            hipLaunchKernelGGL(merge_flag_kernel, dim3(grid_for(n_short)), dim3(256), 0, s, n_short,
                               fold ? fold_mode : (plan.merge ? 1 : 0), rows.skey.p, srow, rowstart, rp.ploc.p, rp.pmask.p, head.p);
            if (fold) {
                DevBuf<uint32_t> hpos;
                GBRS_TRY(hpos.alloc(n_short));
                hipLaunchKernelGGL(run_head_pos_kernel, dim3(grid_for(n_short)), dim3(256), 0, s, n_short, head.p, hincl.p);
                GBRS_TRY(running_max(b.sc, hincl.p, hpos.p, n_short, s));
                hipLaunchKernelGGL(run_cut_kernel, dim3(grid_for(n_short)), dim3(256), 0, s, n_short, FOLD_CAP, hpos.p, head.p);
                GBRS_HIP_CHECK(hipStreamSynchronize(s));      // hpos goes out of scope
            }
            GBRS_TRY(scan_heads(b.sc, head.p, hincl.p, n_short, m32, s));
            if (!fold) break;
            unsigned long long folded_two = 0;
            if (fold_mode == 3) {
                if (!two_total.p) GBRS_TRY(two_total.alloc(1));
                GBRS_HIP_CHECK(hipMemsetAsync(two_total.p, 0, 8, s));
                hipLaunchKernelGGL(folded_two_kernel, dim3(grid_for(n_short)), dim3(256), 0, s, n_short, head.p, srow, rowstart,
                                   two_total.p);
                GBRS_HIP_CHECK(hipMemcpyAsync(&folded_two, two_total.p, 8, hipMemcpyDeviceToHost, s));
                GBRS_HIP_CHECK(hipStreamSynchronize(s));
            }
            const uint64_t words_in = out.n_pairs - b.hf.long_pairs, folded_rows = n_short - m32;
            if (em_take_fold(plan, words_in, folded_rows + folded_two)) { out.n_folded = folded_rows - folded_two; out.n_folded_two = folded_two; break; }
            if (fold_mode == 3) fold_mode = 2;     // the flags again: the one-word fold alone,
            else fold = false;                     // then one row per read
        }
        lr.M = m32;
        GBRS_TRY(lr.hrow.alloc(lr.M));
        if (fold) {
            GBRS_TRY(lr.repeat.alloc(lr.M));
            GBRS_HIP_CHECK(hipMemsetAsync(lr.repeat.p, 0, lr.repeat.bytes(), s));
        }
        if (out.weighted) {
            GBRS_TRY(out.row_weight.alloc(lr.M));
            GBRS_HIP_CHECK(hipMemsetAsync(out.row_weight.p, 0, out.row_weight.bytes(), s));
        }
        hipLaunchKernelGGL(merged_rows_kernel, dim3(grid_for(n_short)), dim3(256), 0, s, n_short, head.p, hincl.p, srow,
                           rp.row_orig.p, count, lr.hrow.p, out.weighted ? out.row_weight.p : nullptr,
                           fold ? lr.repeat.p : (uint32_t *)nullptr);
        GBRS_HIP_CHECK(hipStreamSynchronize(s));
    }
    rows.skey.release();
    lr.fold = fold;
    out.n_rows = lr.M;
    return GBRS_OK;
}

// 6. long rows keep their pair form
int long_rows(Build &b, TileLayout &out, const RowPairs &rp, const SortedRows &rows, const double *count, bool keep_row_ids,
              const EmPlan &plan) {
    hipStream_t s = b.s;
    const uint64_t n_long = rows.n_long, n_short = rows.n_short;
    DevBuf<uint64_t> llen;
    GBRS_TRY(llen.alloc(n_long));
    GBRS_TRY(out.long_ptr.alloc(n_long + 1));
    GBRS_TRY(out.long_weight.alloc(n_long));
    if (keep_row_ids) GBRS_TRY(out.long_row.alloc(n_long));
    hipLaunchKernelGGL(long_rows_kernel, dim3(grid_for(n_long)), dim3(256), 0, s, n_long, n_short, rows.srow.p, rp.rowstart.p,
                       rp.row_orig.p, count, llen.p, out.long_weight.p, keep_row_ids ? out.long_row.p : (uint32_t *)nullptr);
    uint64_t tot = 0;
    GBRS_TRY(scan_total(b.sc, llen.p, out.long_ptr.p, n_long, tot, s, true));
    GBRS_TRY(out.long_loc.alloc(tot)); GBRS_TRY(out.long_mask.alloc(tot));
    hipLaunchKernelGGL(long_copy_kernel, dim3((unsigned)n_long), dim3(64), 0, s, n_long, n_short, rows.srow.p, rp.rowstart.p,
                       rp.ploc.p, rp.pmask.p, out.long_ptr.p, out.long_loc.p, out.long_mask.p);
    GBRS_TRY(out.acc_extra.alloc((size_t)plan.tL * plan.tH));
    GBRS_HIP_CHECK(hipStreamSynchronize(s));
    return GBRS_OK;
}

// the layout's rows cut into T tiles: npm[i] words of row i from word wordoff[i] on, in tile tincl[i] - 1; rows
// tile_row[t] .. tile_row[t + 1] are tile t's
struct Tiles {
    DevBuf<uint32_t> npm, dnew, wordoff, tflag, tincl, tile_row;     // (dnew and tflag: steps 7 and 7b only)
    uint64_t T = 0;
    void release() { tincl.release(); npm.release(); wordoff.release(); tile_row.release(); }
};

// 7 (plan.exact_cut). One rule: a tile ends at tile_words words or at d_max distinct ids, whichever comes first, and the
// next starts fresh.  A pass cuts candidates on the word grid, counts each candidate's distinct ids the way stage 9 will
// (one sort of (candidate, id) keys over the W words) and splits only the candidates above d_max (cut_flag_kernel).  A
// pass that ends above plan.tile_target tiles is repeated at a size larger in proportion (em_plan.h), TILE_CUT_PASSES
// times at most; the pass with the fewest tiles stands.  Fills t.tflag / t.tincl, T: the tiles.
int cut_tiles_exact(Build &b, TileLayout &out, const RowPairs &rp, const LayoutRows &lr, Tiles &t, const EmPlan &plan,
                    uint32_t W, uint32_t &T) {
    hipStream_t s = b.s;
    const uint64_t M = lr.M;
    DevBuf<uint32_t> fresh, fincl, cflag, cincl, cnt, dflag, kept;
    DevBuf<uint64_t> key, key2;
    GBRS_TRY(fresh.alloc(M)); GBRS_TRY(fincl.alloc(M)); GBRS_TRY(cflag.alloc(M)); GBRS_TRY(cincl.alloc(M));
    GBRS_TRY(key.alloc(W)); GBRS_TRY(key2.alloc(W)); GBRS_TRY(dflag.alloc(W));
    hipLaunchKernelGGL(row_new_ids_kernel, dim3(grid_for(M)), dim3(256), 0, s, M, lr.hrow.p, rp.rowstart.p, rp.ploc.p, fresh.p);
    GBRS_TRY(inclusive_scan(b.sc, fresh.p, fincl.p, M, s));
    uint32_t tw = em_cut_tile_words(plan, W), kept_T = 0;
    for (int pass = 1;; ++pass) {
        uint32_t C = 0;
        hipLaunchKernelGGL(cand_flag_kernel, dim3(grid_for(M)), dim3(256), 0, s, M, tw, t.wordoff.p, cflag.p);
        GBRS_TRY(scan_heads(b.sc, cflag.p, cincl.p, M, C, s));
        GBRS_TRY(cnt.alloc(C));
        GBRS_HIP_CHECK(hipMemsetAsync(cnt.p, 0, cnt.bytes(), s));
        hipLaunchKernelGGL(tile_pair_keys_kernel, dim3(grid_for(M)), dim3(256), 0, s, M, cincl.p, lr.hrow.p, rp.rowstart.p, rp.ploc.p,
                           t.wordoff.p, key.p);
        GBRS_TRY(sort_keys64(b.sc, key.p, key2.p, W, 32 + bits_for(C), s));
        hipLaunchKernelGGL(dict_flag_kernel, dim3(grid_for(W)), dim3(256), 0, s, (uint64_t)W, key2.p, dflag.p);
        hipLaunchKernelGGL(cand_count_kernel, dim3(grid_for(W)), dim3(256), 0, s, (uint64_t)W, key2.p, dflag.p, cnt.p);
        hipLaunchKernelGGL(cut_flag_kernel, dim3(grid_for(M)), dim3(256), 0, s, M, plan.dseg, plan.d_max, cflag.p, cincl.p, cnt.p,
                           fincl.p, t.tflag.p);
        GBRS_TRY(scan_heads(b.sc, t.tflag.p, t.tincl.p, M, T, s));
        out.cut_passes = (uint32_t)pass;
        const uint32_t next = em_cut_rescale(plan, tw, T);
        const bool last = next == tw || pass == TILE_CUT_PASSES;
        if (kept_T == 0 || T < kept_T) {
            kept_T = T;
            out.cut_tile_words = tw;
            if (!last) {       // (a later pass may do worse: more of its larger candidates pass d_max)
                if (!kept.p) GBRS_TRY(kept.alloc(M));
                GBRS_HIP_CHECK(hipMemcpyAsync(kept.p, t.tflag.p, M * 4, hipMemcpyDeviceToDevice, s));
            }
        } else if (last) {
            GBRS_HIP_CHECK(hipMemcpyAsync(t.tflag.p, kept.p, M * 4, hipMemcpyDeviceToDevice, s));
            GBRS_TRY(scan_heads(b.sc, t.tflag.p, t.tincl.p, M, T, s));
        }
        if (last) break;
        tw = next;
    }
    GBRS_HIP_CHECK(hipStreamSynchronize(s));
    return GBRS_OK;
}

// 7. tiles
int cut_tiles(Build &b, TileLayout &out, const RowPairs &rp, const LayoutRows &lr, Tiles &t, const EmPlan &plan) {
    hipStream_t s = b.s;
    const uint64_t M = lr.M;
    DevBuf<uint32_t> dincl;
    GBRS_TRY(t.npm.alloc(M)); GBRS_TRY(t.dnew.alloc(M)); GBRS_TRY(t.wordoff.alloc(M)); GBRS_TRY(dincl.alloc(M));
    GBRS_TRY(t.tflag.alloc(M)); GBRS_TRY(t.tincl.alloc(M));
    hipLaunchKernelGGL(row_len_kernel, dim3(grid_for(M)), dim3(256), 0, s, M, lr.hrow.p, rp.rowstart.p, rp.ploc.p, t.npm.p, t.dnew.p);
    GBRS_TRY(exclusive_scan(b.sc, t.npm.p, t.wordoff.p, M, s));
    GBRS_TRY(inclusive_scan(b.sc, t.dnew.p, dincl.p, M, s));
    uint32_t total_words = 0;
    GBRS_TRY(fetch_last_plus(t.wordoff.p, t.npm.p, M, total_words, s));
    out.all_one_word = total_words == M && out.n_long == 0;
    uint32_t T32 = 0;
    out.cut_passes = 0;
    out.cut_tile_words = em_tile_words(plan, total_words);
    if (em_take_exact_cut(plan, total_words)) {
        dincl.release();
        GBRS_TRY(cut_tiles_exact(b, out, rp, lr, t, plan, total_words, T32));
    } else {
        hipLaunchKernelGGL(tile_flag_kernel, dim3(grid_for(M)), dim3(256), 0, s, M, out.cut_tile_words, plan.dseg, t.npm.p,
                           t.wordoff.p, dincl.p, t.tflag.p);
        GBRS_TRY(scan_heads(b.sc, t.tflag.p, t.tincl.p, M, T32, s));
    }
    t.T = T32;
    out.n_tiles = t.T;
    dincl.release();
    GBRS_TRY(t.tile_row.alloc(t.T + 1));
    hipLaunchKernelGGL(tile_start_kernel, dim3(grid_for(M)), dim3(256), 0, s, M, t.T, t.tflag.p, t.tincl.p, t.tile_row.p);
    return GBRS_OK;
}

// 7b. interleave the locus lists inside each tile, or lay the tile's rows out as streams (tile membership and sizes are
// unchanged)
int order_rows_in_tiles(Build &b, TileLayout &out, LayoutRows &lr, Tiles &t, bool interleave) {
    hipStream_t s = b.s;
    Scratch &sc = b.sc;
    const uint64_t M = lr.M;
    const bool fold = lr.fold;
    DevBuf<uint32_t> gflag, gpos, gstart, gord, ident, perm, hrow2, npm2, repeat2;
    DevBuf<uint64_t> ikey, ikey2;
    DevBuf<double> weight2;
    if (interleave) {
        GBRS_TRY(gflag.alloc(M)); GBRS_TRY(gpos.alloc(M)); GBRS_TRY(gstart.alloc(M)); GBRS_TRY(gord.alloc(M));
        hipLaunchKernelGGL(group_flag_kernel, dim3(grid_for(M)), dim3(256), 0, s, M, t.dnew.p, t.tflag.p, gflag.p, gpos.p);
        GBRS_TRY(running_max(sc, gpos.p, gstart.p, M, s));
        GBRS_TRY(inclusive_scan(sc, gflag.p, gord.p, M, s));
        GBRS_HIP_CHECK(hipStreamSynchronize(s));
        gflag.release(); gpos.release();
    }
    GBRS_TRY(ikey.alloc(M)); GBRS_TRY(ikey2.alloc(M)); GBRS_TRY(ident.alloc(M)); GBRS_TRY(perm.alloc(M));
    b.mark("7b-a alloc");
    if (interleave)
        hipLaunchKernelGGL(interleave_key_kernel, dim3(grid_for(M)), dim3(256), 0, s, M, t.tincl.p, gstart.p, gord.p, ikey.p, ident.p);
    else
        hipLaunchKernelGGL(stream_key_kernel, dim3(grid_for(M)), dim3(256), 0, s, M, t.tincl.p, t.npm.p, ikey.p, ident.p);
    b.mark("7b-b keys");
    GBRS_TRY(sort_pairs<uint64_t>(sc, ikey.p, ikey2.p, ident.p, perm.p, M, 40 + bits_for(t.T), s));
    GBRS_HIP_CHECK(hipStreamSynchronize(s));
    b.mark("7b-c sort");
    ikey.release(); ikey2.release(); ident.release(); gstart.release(); gord.release();
    b.mark("7b-d release");
    GBRS_TRY(hrow2.alloc(M)); GBRS_TRY(npm2.alloc(M));
    if (out.weighted) GBRS_TRY(weight2.alloc(M));
    if (fold) GBRS_TRY(repeat2.alloc(M));
    hipLaunchKernelGGL(permute_rows_kernel, dim3(grid_for(M)), dim3(256), 0, s, M, perm.p, lr.hrow.p, t.npm.p,
                       out.weighted ? out.row_weight.p : (const double *)nullptr, fold ? lr.repeat.p : (const uint32_t *)nullptr,
                       hrow2.p, npm2.p, out.weighted ? weight2.p : (double *)nullptr, fold ? repeat2.p : (uint32_t *)nullptr);
    if (fold) GBRS_HIP_CHECK(hipMemcpyAsync(lr.repeat.p, repeat2.p, M * 4, hipMemcpyDeviceToDevice, s));
    GBRS_HIP_CHECK(hipMemcpyAsync(lr.hrow.p, hrow2.p, M * 4, hipMemcpyDeviceToDevice, s));
    GBRS_HIP_CHECK(hipMemcpyAsync(t.npm.p, npm2.p, M * 4, hipMemcpyDeviceToDevice, s));
    if (out.weighted)
        GBRS_HIP_CHECK(hipMemcpyAsync(out.row_weight.p, weight2.p, M * 8, hipMemcpyDeviceToDevice, s));
    GBRS_TRY(exclusive_scan(sc, t.npm.p, t.wordoff.p, M, s));
    GBRS_HIP_CHECK(hipStreamSynchronize(s));
    return GBRS_OK;
}

// per row its padding, per tile its batches and where its dictionary starts
struct TileParts {
    DevBuf<uint32_t> rowpad, nbatch, n_one, n_two, batch_base, dict_base;
    uint32_t NB = 0, NS = 0;     // batches and dictionary entries (slots) of the layout
    void release() { dict_base.release(); batch_base.release(); nbatch.release(); n_one.release(); n_two.release(); rowpad.release(); }
};

// 8. padding so that no row straddles a batch, batch offsets
int pad_rows(Build &b, TileLayout &out, const RowPairs &rp, const LayoutRows &lr, const Tiles &t, TileParts &tp,
             const EmPlan &plan) {
    hipStream_t s = b.s;
    const uint64_t T = t.T, M = lr.M;
    GBRS_TRY(tp.rowpad.alloc(M)); GBRS_TRY(tp.nbatch.alloc(T)); GBRS_TRY(tp.n_one.alloc(T)); GBRS_TRY(tp.n_two.alloc(T));
    GBRS_TRY(tp.batch_base.alloc(T));
    // stripes (em_plan.h): where the layout takes them, the rows that start a group
    DevBuf<uint8_t> head;
    uint32_t W = 0;
    if (plan.counted_pairs && (plan.stripes_one != 0 || plan.stripes_two != 0)) GBRS_TRY(fetch_last_plus(t.wordoff.p, t.npm.p, M, W, s));
    out.stripes = em_take_stripes(plan, W);
    if (out.stripes) {
        GBRS_TRY(head.alloc(M));
        hipLaunchKernelGGL(stripe_head_kernel, dim3(grid_for(M)), dim3(256), 0, s, M, t.npm.p, lr.hrow.p, rp.rowstart.p, rp.ploc.p, head.p);
    }
    hipLaunchKernelGGL(tile_pad_kernel, dim3(grid_for(T, 64)), dim3(64), 0, s, T, plan.row_order == 2 ? 1 : 0, t.tile_row.p, t.npm.p,
                       tp.rowpad.p, tp.nbatch.p, tp.n_one.p, tp.n_two.p, out.stripes ? head.p : (const uint8_t *)nullptr,
                       plan.stripes_one, plan.stripes_two);
    // (the weighted kernels do not split their batch loop: their headers say nothing about the leading batches)
    if (out.weighted) GBRS_HIP_CHECK(hipMemsetAsync(tp.n_one.p, 0, T * 4, s));
    if (!plan.counted_pairs) GBRS_HIP_CHECK(hipMemsetAsync(tp.n_two.p, 0, T * 4, s));
    GBRS_TRY(scan_total(b.sc, tp.nbatch.p, tp.batch_base.p, T, tp.NB, s));
    out.n_batches = tp.NB;
    return GBRS_OK;
}

// 9. per-tile dictionaries: one sort of (tile, id) keys over all the pairs (see tile_pair_keys_kernel)
int tile_dictionaries(Build &b, TileLayout &out, const RowPairs &rp, const LayoutRows &lr, const Tiles &t, TileParts &tp) {
    hipStream_t s = b.s;
    const uint64_t M = lr.M, T = t.T;
    GBRS_TRY(tp.dict_base.alloc(T));
    uint32_t W = 0;
    GBRS_TRY(fetch_last_plus(t.wordoff.p, t.npm.p, M, W, s));
    DevBuf<uint64_t> dkey, dkey2;
    DevBuf<uint32_t> dflag, dpos;
    GBRS_TRY(dkey.alloc(W)); GBRS_TRY(dkey2.alloc(W)); GBRS_TRY(dflag.alloc(W)); GBRS_TRY(dpos.alloc(W));
    hipLaunchKernelGGL(tile_pair_keys_kernel, dim3(grid_for(M)), dim3(256), 0, s, M, t.tincl.p, lr.hrow.p, rp.rowstart.p, rp.ploc.p,
                       t.wordoff.p, dkey.p);
    GBRS_TRY(sort_keys64(b.sc, dkey.p, dkey2.p, W, 32 + bits_for(T), s));
    hipLaunchKernelGGL(dict_flag_kernel, dim3(grid_for(W)), dim3(256), 0, s, (uint64_t)W, dkey2.p, dflag.p);
    GBRS_TRY(scan_total(b.sc, dflag.p, dpos.p, W, tp.NS, s));
    out.n_slots = tp.NS;
    GBRS_TRY(out.tiles.alloc(T));
    GBRS_TRY(out.dict.alloc(std::max<uint32_t>(tp.NS, 1)));
    hipLaunchKernelGGL(dict_emit_kernel, dim3(grid_for(W)), dim3(256), 0, s, (uint64_t)W, dkey2.p, dflag.p, dpos.p, out.dict.p,
                       tp.dict_base.p);
    hipLaunchKernelGGL(tile_hdr_kernel, dim3(grid_for(T)), dim3(256), 0, s, T, out.d_max, tp.NS, tp.batch_base.p, tp.nbatch.p,
                       tp.n_one.p, tp.n_two.p, tp.dict_base.p, out.tiles.p, b.d_flags.p);
    GBRS_TRY(b.read_flags());
    if (b.hf.dict_overflow) return fail(GBRS_ERR_INVALID, "internal error: a tile dictionary overflowed its capacity");
    return GBRS_OK;
}

// 10. words
int emit_words(Build &b, TileLayout &out, const RowPairs &rp, const LayoutRows &lr, const Tiles &t, const TileParts &tp,
               bool keep_row_ids, const EmPlan &plan) {
    hipStream_t s = b.s;
    const uint64_t M = lr.M, T = t.T;
    GBRS_TRY(out.words.alloc((size_t)tp.NB * 64));
    GBRS_HIP_CHECK(hipMemsetAsync(out.words.p, 0, out.words.bytes(), s));
    if (out.weighted) {
        GBRS_TRY(out.word_weight.alloc((size_t)tp.NB * 64));
        GBRS_HIP_CHECK(hipMemsetAsync(out.word_weight.p, 0, out.word_weight.bytes(), s));
    }
    if (keep_row_ids) {
        GBRS_TRY(out.word_row.alloc((size_t)tp.NB * 64));
        GBRS_HIP_CHECK(hipMemsetAsync(out.word_row.p, 0xFF, out.word_row.bytes(), s));      // padding cells: no row
    }
    hipLaunchKernelGGL(emit_words_kernel, dim3(grid_for(M)), dim3(256), 0, s, M, plan.tH, t.tincl.p, out.tiles.p, out.dict.p,
                       lr.hrow.p, rp.rowstart.p, rp.ploc.p, rp.pmask.p, tp.rowpad.p, out.words.p,
                       out.weighted ? out.row_weight.p : (const double *)nullptr,
                       out.weighted ? out.word_weight.p : (double *)nullptr,
                       keep_row_ids ? rp.row_orig.p : (const uint32_t *)nullptr, keep_row_ids ? out.word_row.p : (uint32_t *)nullptr,
                       lr.fold ? lr.repeat.p : (const uint32_t *)nullptr);
    if (plan.row_order == 2 && !out.weighted)
        hipLaunchKernelGGL(fill_one_word_cells_kernel, dim3(grid_for(T * 64)), dim3(256), 0, s, T, plan.tH, out.tiles.p, out.words.p);
    GBRS_HIP_CHECK(hipStreamSynchronize(s));
    return GBRS_OK;
}

// Launch order of the tiles: the ones with the most batches first, so that the launch's last round - when most
// of the chip has run out of tiles - is made of the short ones (tiles that end at the dictionary limit have
// fewer words; C2: E-step 0.0998-0.1008 -> 0.0960-0.0962 ms).  Nothing but the E-step reads the header array by
// position.  GBRS_TUNING_TILE_ORDER=0 keeps the locus order.
int reorder_tiles(TileLayout &out, uint64_t T) {
    std::vector<TileHdr> hdr(T);
    GBRS_HIP_CHECK(hipMemcpy(hdr.data(), out.tiles.p, T * sizeof(TileHdr), hipMemcpyDeviceToHost));
    std::stable_sort(hdr.begin(), hdr.end(), [](const TileHdr &a, const TileHdr &b) { return a.n_batches > b.n_batches; });
    GBRS_HIP_CHECK(hipMemcpy(out.tiles.p, hdr.data(), T * sizeof(TileHdr), hipMemcpyHostToDevice));
    return GBRS_OK;
}

// 11. inverted index locus -> destination rows.  A slot (tile, dictionary entry) of a locus delivers one row of sums
// to that locus; the slot of a locus set delivers the same row to every member locus.  The rows are numbered by
// locus (ascending slot inside a locus: the radix sort is stable), so that the rows of a locus are consecutive in
// `partials` and the gather streams them without an indirection.
int inverted_index(Build &b, TileLayout &out, uint32_t NS, uint32_t L_in, uint32_t H) {
    hipStream_t s = b.s;
    GBRS_TRY(out.slot_dest.alloc(std::max<uint32_t>(NS, 1)));
    uint32_t NE = 0, n_rows_real = 0;
    if (NS) {
        DevBuf<uint32_t> ecnt, eoff;
        GBRS_TRY(ecnt.alloc(NS)); GBRS_TRY(eoff.alloc(NS));
        hipLaunchKernelGGL(dest_count_kernel, dim3(grid_for(NS)), dim3(256), 0, s, (uint64_t)NS, L_in, out.dict.p,
                           out.n_sets ? out.set_ptr.p : (const uint32_t *)nullptr, ecnt.p);
        GBRS_TRY(scan_total(b.sc, ecnt.p, eoff.p, NS, NE, s));
        // (SLOT_PAIR is the lowest flag bit of a destination: checked here, before anything is sized by NE or indexed with it)
        if (NE >= SLOT_PAIR) return fail(GBRS_ERR_INVALID, "the tiled layout needs fewer than 2^29 destination rows");
        DevBuf<uint32_t> eloc, eidx, sloc;
        GBRS_TRY(eloc.alloc(NE)); GBRS_TRY(eidx.alloc(NE)); GBRS_TRY(sloc.alloc(NE));
        GBRS_TRY(out.slot_list.alloc(NE));
        GBRS_TRY(out.dest_list.alloc(NE));
        hipLaunchKernelGGL(dest_emit_kernel, dim3(grid_for(NS)), dim3(256), 0, s, (uint64_t)NS, L_in, out.dict.p,
                           out.n_sets ? out.set_ptr.p : (const uint32_t *)nullptr, out.set_members.p, eoff.p, eloc.p, eidx.p,
                           out.slot_dest.p, out.dest_list.p);
        // (the header entry of a set slot carries locus id L_in: behind every real locus, never looked at)
        GBRS_TRY(sort_pairs<uint32_t>(b.sc, eloc.p, sloc.p, eidx.p, out.slot_list.p, NE, bits_for(L_in), s));
        hipLaunchKernelGGL(slot_ptr_kernel, dim3(grid_for((uint64_t)L_in + 1)), dim3(256), 0, s, L_in, (uint64_t)NE, sloc.p,
                           out.slot_ptr.p);
        // the rows that receive sums: the entries of real loci (a set slot's header entry sorts behind them)
        GBRS_HIP_CHECK(hipMemcpyAsync(&n_rows_real, out.slot_ptr.p + L_in, 4, hipMemcpyDeviceToHost, s));
        GBRS_HIP_CHECK(hipStreamSynchronize(s));
    } else {
        GBRS_TRY(out.slot_list.alloc(1));
        GBRS_TRY(out.dest_list.alloc(1));
    }
    out.n_dest_rows = n_rows_real;
    GBRS_TRY(out.partials.alloc(std::max<size_t>((size_t)n_rows_real * H, 1)));
    hipLaunchKernelGGL(locus_class_kernel, dim3(grid_for(L_in)), dim3(256), 0, s, L_in, out.slot_ptr.p, out.slot_list.p,
                       out.locus_class.p, out.dest_list.p);
    if (NS) hipLaunchKernelGGL(dest_route_kernel, dim3(grid_for(NS)), dim3(256), 0, s, (uint64_t)NS, out.dest_list.p, out.slot_dest.p);
    if (out.n_sets && NS) {
        GBRS_TRY(out.dict_b.alloc(NS));
        GBRS_TRY(out.dest_b.alloc(NS));
        hipLaunchKernelGGL(encode_sets_kernel, dim3(grid_for(NS)), dim3(256), 0, s, (uint64_t)NS, L_in, out.set_ptr.p,
                           out.set_members.p, out.dest_list.p, out.dict.p, out.dict_b.p, out.slot_dest.p, out.dest_b.p);
    }
    return GBRS_OK;
}

// 12. loci with many slots get a whole wave in the gather kernel
int heavy_light_lists(TileLayout &out, uint32_t L_in, hipStream_t s) {
    std::vector<uint32_t> sp((size_t)L_in + 1), heavy, lightv;
    GBRS_HIP_CHECK(hipMemcpyAsync(sp.data(), out.slot_ptr.p, sp.size() * 4, hipMemcpyDeviceToHost, s));
    GBRS_HIP_CHECK(hipStreamSynchronize(s));
    for (uint32_t l = 0; l < L_in; ++l)
        if (sp[l + 1] - sp[l] > (uint32_t)HEAVY_SLOTS) heavy.push_back(l);
        else if (sp[l + 1] - sp[l] >= 2) lightv.push_back(l);
    out.n_heavy = heavy.size();
    out.n_light = lightv.size();
    for (int which = 0; which < 2; ++which) {
        const std::vector<uint32_t> &loci = which == 0 ? heavy : lightv;
        DevBuf<uint32_t> &dst = which == 0 ? out.heavy_range : out.light_range;
        std::vector<uint32_t> rng;
        rng.reserve(loci.size() * 3);
        for (uint32_t l : loci) {
            rng.push_back(l);
            rng.push_back(sp[l]);
            rng.push_back(sp[l + 1]);
        }
        GBRS_TRY(dst.alloc(std::max<size_t>(rng.size(), 3)));
        if (!rng.empty()) GBRS_HIP_CHECK(hipMemcpyAsync(dst.p, rng.data(), rng.size() * 4, hipMemcpyHostToDevice, s));
        GBRS_HIP_CHECK(hipStreamSynchronize(s));          // rng goes out of scope
    }
    GBRS_TRY(out.light_loci.alloc(std::max<size_t>(lightv.size(), 1)));
    if (!lightv.empty())
        GBRS_HIP_CHECK(hipMemcpyAsync(out.light_loci.p, lightv.data(), lightv.size() * 4, hipMemcpyHostToDevice, s));
    GBRS_TRY(out.heavy_loci.alloc(std::max<size_t>(heavy.size(), 1)));
    if (!heavy.empty())
        GBRS_HIP_CHECK(hipMemcpyAsync(out.heavy_loci.p, heavy.data(), heavy.size() * 4, hipMemcpyHostToDevice, s));
    GBRS_HIP_CHECK(hipStreamSynchronize(s));
    return GBRS_OK;
}

}  // namespace

// 13. the gather-side M-step's words (em_layout.h, GatherArgs): the locus of every (slot, member) with its owner and
// direct flags, beside slot_dest, dest_b and dest_list.  The owner of a locus is its first (slot, member) in slot order,
// members in member order; a locus is direct when that is its only one.  On the host: once per handle, a few words per slot.
int build_gather_slots(TileLayout &tl, uint32_t L, hipStream_t s) {
    if (tl.gather_slots) return GBRS_OK;
    const size_t NS = tl.n_slots;
    const bool sets = tl.n_sets != 0;
    std::vector<uint32_t> dict(NS), dict_b, sdest, set_ptr, members;
    std::vector<uint32_t> gdest(std::max<size_t>(NS, 1), 0u), gdest_b, glist(std::max<size_t>(tl.dest_list.n, 1), 0u);
    GBRS_HIP_CHECK(hipStreamSynchronize(s));
    if (NS) GBRS_HIP_CHECK(hipMemcpy(dict.data(), tl.dict.p, NS * 4, hipMemcpyDeviceToHost));
    if (sets && NS) {
        dict_b.resize(NS); sdest.resize(NS); gdest_b.assign(NS, 0u);
        set_ptr.resize((size_t)tl.n_sets + 1); members.resize(tl.set_members.n);
        GBRS_HIP_CHECK(hipMemcpy(dict_b.data(), tl.dict_b.p, NS * 4, hipMemcpyDeviceToHost));
        GBRS_HIP_CHECK(hipMemcpy(sdest.data(), tl.slot_dest.p, NS * 4, hipMemcpyDeviceToHost));
        GBRS_HIP_CHECK(hipMemcpy(set_ptr.data(), tl.set_ptr.p, set_ptr.size() * 4, hipMemcpyDeviceToHost));
        if (!members.empty()) GBRS_HIP_CHECK(hipMemcpy(members.data(), tl.set_members.p, members.size() * 4, hipMemcpyDeviceToHost));
    }
    // every (slot, member) in order: fn(locus, where its word goes)
    auto walk = [&](auto &&fn) -> int {
        for (size_t p = 0; p < NS; ++p) {
            const uint32_t e = dict[p];
            if (!sets || !(e & (DICT_PAIR | DICT_SET))) {
                if (e >= L) return fail(GBRS_ERR_STATE, "a dictionary entry is no locus");
                fn(e, gdest[p]);
            } else if (e & DICT_PAIR) {
                const uint32_t a = e & ~DICT_PAIR, b2 = dict_b[p];
                if (a >= L || b2 >= L) return fail(GBRS_ERR_STATE, "a two-member set's entry is no locus");
                fn(a, gdest[p]);
                fn(b2, gdest_b[p]);
            } else {
                const uint32_t k = e & ~DICT_SET;
                if (k >= tl.n_sets || !(sdest[p] & SLOT_SET)) return fail(GBRS_ERR_STATE, "a set entry without a destination list");
                const size_t off = sdest[p] & ~SLOT_SET, m0 = set_ptr[k], n = set_ptr[k + 1] - m0;
                if (off + n >= glist.size() || m0 + n > members.size()) return fail(GBRS_ERR_STATE, "a set's destination list is out of range");
                glist[off] = (uint32_t)n;
                for (size_t q = 0; q < n; ++q) {
                    if (members[m0 + q] >= L) return fail(GBRS_ERR_STATE, "a set member is no locus");
                    fn(members[m0 + q], glist[off + 1 + q]);
                }
            }
        }
        return GBRS_OK;
    };
    std::vector<uint32_t> uses(L, 0u);
    GBRS_TRY(walk([&](uint32_t l, uint32_t &) { ++uses[l]; }));
    std::vector<uint8_t> owned(L, 0);
    GBRS_TRY(walk([&](uint32_t l, uint32_t &w) {
        w = l | (owned[l] ? 0u : GSLOT_OWNER) | (uses[l] == 1 ? GSLOT_DIRECT : 0u);
        owned[l] = 1;
    }));
    GBRS_TRY(tl.gdest.alloc(gdest.size()));
    GBRS_TRY(tl.gdest_b.alloc(std::max<size_t>(gdest_b.size(), 1)));
    GBRS_TRY(tl.gdest_list.alloc(glist.size()));
    GBRS_HIP_CHECK(hipMemcpy(tl.gdest.p, gdest.data(), gdest.size() * 4, hipMemcpyHostToDevice));
    if (!gdest_b.empty()) GBRS_HIP_CHECK(hipMemcpy(tl.gdest_b.p, gdest_b.data(), gdest_b.size() * 4, hipMemcpyHostToDevice));
    GBRS_HIP_CHECK(hipMemcpy(tl.gdest_list.p, glist.data(), glist.size() * 4, hipMemcpyHostToDevice));
    tl.gather_slots = true;
    return GBRS_OK;
}

int build_tile_layout(TileLayout &out, uint64_t R, uint64_t N, const uint32_t *ent_row, const uint64_t *col_ptr,
                      const double *count, hipStream_t s, const EmPlan &plan) {
    const uint32_t L_in = plan.tL, H = plan.tH;
    out.n_sets = 0;
    out.n_dest_rows = 0;
    const bool keep_row_ids = out.keep_row_ids && !plan.merge;      // (a merged row has no single file row)
    if (H > 16) return fail(GBRS_ERR_INVALID, "the tiled layout packs the haplotype mask in 16 bits (H <= 16)");
    if (N >= 0xFFFFFFFFull || L_in >= (1u << 27))
        return fail(GBRS_ERR_INVALID, "the tiled layout needs N < 2^32 entries and L < 2^27 loci per handle");
    // (common.h) the temporaries are parked while the build runs - a hipMalloc that follows a large hipFree stalls on
    // some hosts - and go back in one pass when it ends; a one-shot process leaves them to the layout's destructor
    DeferFrees park_temporaries(out.retain_temporaries ? &out.retired : nullptr, &out.retired_bytes);
    StageTimer stg("layout");
    Build b(s, &stg);
    GBRS_TRY(b.init());
    out.d_max = plan.d_max;
    out.deterministic = plan.deterministic;
    if (!plan.dict_room)
        return fail(GBRS_ERR_UNSUPPORTED, "the deterministic tile layout has no room for a row's loci at H = %u", H);
    out.weighted = plan.weighted;
    out.n_pairs = out.n_rows = out.n_rows_in = out.n_long = out.n_tiles = out.n_batches = out.n_slots = out.n_folded = out.n_folded_two = 0;
    GBRS_TRY(out.slot_ptr.alloc((size_t)L_in + 1));
    GBRS_HIP_CHECK(hipMemsetAsync(out.slot_ptr.p, 0, out.slot_ptr.bytes(), s));
    GBRS_TRY(out.locus_class.alloc(L_in));
    GBRS_HIP_CHECK(hipMemsetAsync(out.locus_class.p, 0, out.locus_class.bytes(), s));
    if (N == 0) { GBRS_HIP_CHECK(hipStreamSynchronize(s)); return GBRS_OK; }

    // 1-3. entries -> pairs -> rows
    RowPairs rp;
    stg.mark("0 setup");
    GBRS_TRY(build_row_pairs(b, rp, R, L_in, H, N, ent_row, col_ptr, 5 + bits_for(L_in - 1) /* <= 32: L < 2^27 */, plan.view));
    out.n_pairs = rp.P;
    out.n_rows_in = rp.R1;
    stg.mark("3 rows");
    // 3b, 3c. locus sets
    if (plan.whole_row_sets && rp.R1 > 0) {
        GBRS_TRY(whole_row_sets(b, out, rp, plan));
        stg.mark("3b locus sets");
    }
    if (plan.locus_sets && rp.R1 > 0 && out.n_sets == 0) {
        if (plan.group_sets) GBRS_TRY(mask_group_sets(b, out, rp, plan));
        stg.mark("3c mask-group sets");
    }
    // 4-6. the rows in their order, merged or folded; the long ones apart
    SortedRows rows;
    LayoutRows lr;
    GBRS_TRY(order_rows(b, out, rp, rows, L_in + out.n_sets, H));
    stg.mark("4 order rows");
    GBRS_TRY(merge_rows(b, out, rp, rows, lr, count, plan));
    out.all_one_word = false;
    stg.mark("5 merge");
    if (rows.n_long) GBRS_TRY(long_rows(b, out, rp, rows, count, keep_row_ids, plan));
    rows.srow.release();
    if (!keep_row_ids) rp.row_orig.release();      // (a resampling handle's words remember their file rows: emit_words_kernel)
    if (lr.M == 0) { GBRS_HIP_CHECK(hipStreamSynchronize(s)); return GBRS_OK; }
    stg.mark("6 long rows");
    // 7-10. tiles, their row order, batches, dictionaries and words
    Tiles tiles;
    TileParts parts;
    GBRS_TRY(cut_tiles(b, out, rp, lr, tiles, plan));
    stg.mark("7 tiles");
    if (plan.row_order != 0) GBRS_TRY(order_rows_in_tiles(b, out, lr, tiles, plan.row_order == 1));
    tiles.dnew.release();
    tiles.tflag.release();
    stg.mark("7b row order");
    GBRS_TRY(pad_rows(b, out, rp, lr, tiles, parts, plan));
    stg.mark("8 padding");
    GBRS_TRY(tile_dictionaries(b, out, rp, lr, tiles, parts));
    stg.mark("9 dictionaries");
    GBRS_TRY(emit_words(b, out, rp, lr, tiles, parts, keep_row_ids, plan));
    parts.release(); tiles.release(); lr.release(); rp.release();
    out.row_weight.release();
    if (plan.reorder_tiles && tiles.T > 1) GBRS_TRY(reorder_tiles(out, tiles.T));
    stg.mark("10 words");
    // 11-12. what the gather reads
    GBRS_TRY(inverted_index(b, out, parts.NS, L_in, H));
    stg.mark("11 inverted index");
    GBRS_TRY(heavy_light_lists(out, L_in, s));
    stg.mark("12 heavy / light lists");
    GBRS_HIP_CHECK(hipGetLastError());
    return GBRS_OK;
}

}  // namespace gbrs

// ---- grouped row layout of multiread models 1-3 ----------------------------------------------------------------------
namespace gbrs {
namespace {

__global__ void __launch_bounds__(256)
row_hist_kernel(uint64_t n, const uint32_t *__restrict__ ent_row, uint32_t *__restrict__ cnt) {
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n) atomicAdd(&cnt[ent_row[k]], 1u);
}

// key = row << rank_bits | rank[column], value = the entry's CSC index
__global__ void __launch_bounds__(256)
grouped_key_kernel(uint64_t n, uint32_t ncols, const uint64_t *__restrict__ col_ptr, const uint32_t *__restrict__ ent_row,
                   const uint32_t *__restrict__ rank, unsigned rank_bits, uint64_t *__restrict__ key,
                   uint32_t *__restrict__ val) {
    const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k - (threadIdx.x & 63) >= n) return;
    const bool live = k < n;
    const uint32_t c = entry_column(col_ptr, ncols, live ? k : n - 1, n);
    if (!live) return;
    key[k] = ((uint64_t)ent_row[k] << rank_bits) | rank[c];
    val[k] = (uint32_t)k;
}

__global__ void __launch_bounds__(256)
grouped_lh_kernel(uint64_t n, const uint64_t *__restrict__ key, uint64_t mask, const uint32_t *__restrict__ rank_lh,
                  uint32_t *__restrict__ lh) {
    const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j < n) lh[j] = rank_lh[key[j] & mask];
}

}  // namespace

int build_row_ptr(DevBuf<uint32_t> &row_ptr, uint64_t R, uint64_t N, const uint32_t *ent_row, hipStream_t s) {
    Scratch sc;
    DevBuf<uint32_t> cnt;
    GBRS_TRY(cnt.alloc(R + 1));
    GBRS_TRY(row_ptr.alloc(R + 1));
    GBRS_HIP_CHECK(hipMemsetAsync(cnt.p, 0, cnt.bytes(), s));
    if (N) hipLaunchKernelGGL(row_hist_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s, N, ent_row, cnt.p);
    GBRS_HIP_CHECK(hipGetLastError());
    GBRS_TRY(exclusive_scan(sc, cnt.p, row_ptr.p, R + 1, s));      // (the last count is 0: row_ptr[R] = N)
    GBRS_HIP_CHECK(hipStreamSynchronize(s));
    return GBRS_OK;
}

int build_grouped_order(GroupedOrder &out, uint64_t R, uint32_t L, uint32_t H, uint64_t N, const uint32_t *ent_row,
                        const uint64_t *col_ptr, const uint32_t *rank, const uint32_t *rank_lh, hipStream_t s) {
    out.built = false;
    if (N >= 0xFFFFFFFFull || L >= (1u << 27))
        return fail(GBRS_ERR_UNSUPPORTED, "the grouped layout holds at most 2^32 - 1 entries of at most 2^27 loci");
    GBRS_TRY(out.lh.alloc(std::max<uint64_t>(N, 1)));
    GBRS_TRY(out.src.alloc(std::max<uint64_t>(N, 1)));
    if (N) {
        const uint32_t ncols = H * L;
        const unsigned rank_bits = bits_for(ncols - 1), end_bit = rank_bits + bits_for(R - 1);
        Scratch sc;
        DevBuf<uint64_t> kin, kout;
        DevBuf<uint32_t> vin;
        GBRS_TRY(kin.alloc(N));
        GBRS_TRY(kout.alloc(N));
        GBRS_TRY(vin.alloc(N));
        const unsigned grid = (unsigned)((N + 255) / 256);
        hipLaunchKernelGGL(grouped_key_kernel, dim3(grid), dim3(256), 0, s, N, ncols, col_ptr, ent_row, rank, rank_bits,
                           kin.p, vin.p);
        GBRS_HIP_CHECK(hipGetLastError());
        GBRS_TRY(sort_pairs(sc, kin.p, kout.p, vin.p, out.src.p, N, end_bit, s));
        hipLaunchKernelGGL(grouped_lh_kernel, dim3(grid), dim3(256), 0, s, N, kout.p, (uint64_t(1) << rank_bits) - 1,
                           rank_lh, out.lh.p);
        GBRS_HIP_CHECK(hipGetLastError());
        GBRS_HIP_CHECK(hipStreamSynchronize(s));
    }
    out.built = true;
    return GBRS_OK;
}

}  // namespace gbrs

// gbrs_warm_up (common.hip): loads this file's code object
namespace gbrs {
__global__ void warm_layout_kernel() {}
void warm_layout(hipStream_t st) { hipLaunchKernelGGL(warm_layout_kernel, dim3(1), dim3(64), 0, st); }
}  // namespace gbrs

// ---- row sharding of one sample over the ranks of `gbrs quantify --gpus N` ---------------------------------------------
#include "em_shard.inc"
