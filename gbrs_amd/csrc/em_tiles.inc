// E-step over the packed-row-tile layout (em_layout.h).  Included by em.hip inside namespace gbrs.
//
// One workgroup = one tile.  The tile's theta (D x H doubles, gathered through the dictionary)
// and its partial sums live in LDS; one wavefront takes one 64-word batch per step:
//   s[lane]   = sum of theta over the haplotypes set in the word's mask          (LDS reads)
//   den       = sum of s over the words of the row (rows never straddle a batch): DPP wave shifts
//   v         = weight / den
//   A[idx][h] += v for every set haplotype: accumulated in the lane's registers while the lane
//               stays on one locus, then LDS float64 atomics into one of K private copies
//               (K = as many copies as fit, up to one per lane, so that a tile dominated by a
//               single hot locus does not serialise on one LDS address)
// then the copies are summed in fixed order and stored as the tile's slots of `partials`
// (plain coalesced stores; no global atomics).

// word decode (em_layout.h): [ idx | rem | pos | mask ]
//   mask  H bits     haplotypes the read aligns to at this locus
//   pos   PB bits    words of the same row to the left of this one
//   rem   PB bits    words of the same row to the right of this one
//   idx              index into the tile's dictionary
// A word without a haplotype bit is padding (a one-word row with no haplotype: contributes nothing): all zero, or - in a
// tile's leading one-word batches - with the dictionary index of the cell above it (TileHdr::n_one).
// In a tile's leading one-word batches (batch index < TileHdr::n_one) pos = rem = 0 by construction, and the 2 PB bits of
// the two fields are ONE field instead: the number of FURTHER identical reads the word stands for (the fold of
// em_layout.h; 0 everywhere in a layout that did not fold, and 0 in padding words).  Such a word adds v = (1 + count) / den.
// Every kernel instance that can meet an unweighted tile of 1, 2, 4 or 8 haplotypes reads those batches that way: the LEAD
// form of tile_batches always, the general form when its caller says `count_form` (wave-uniform: the batch index).
// The batches behind them, index in [n_one, n_one + TileHdr::n_two), hold two-word rows on (even, odd) lane pairs only (or
// padding pairs): the lane's parity is the word's position, the 2 PB bits of BOTH words are the row's repeat count, and
// den = s + s of the partner lane with no vote at all.  The LEAD form takes them under its wave-uniform `pair` argument,
// the general form under count_form = 2.

#ifndef GBRS_ESTEP_WAVES16
#define GBRS_ESTEP_WAVES16 4          // the same for more than 8 haplotypes
#endif
#ifndef GBRS_ESTEP_WAVES
#define GBRS_ESTEP_WAVES 6            // waves per SIMD the unweighted <= 8-haplotype kernel is compiled for (3 workgroups per CU)
#endif
#if !defined(GBRS_NO_MASK_ZLO) && !defined(GBRS_MASK_ZLO)
#define GBRS_MASK_ZLO 1
#endif
// Batches a wavefront works on together.  Two give independent chains (ILP) but twice the live registers;
// the unweighted kernels run one batch at a time at 72 (8 haplotypes) / 126 (16) VGPRs, which with 3,072
// doubles of theta per tile (49 KB of LDS per workgroup) puts three workgroups = 6 waves per SIMD on a CU
// for 8 haplotypes and two = 4 waves per SIMD for 16 (from 4 and 2): E-step 0.150 -> 0.141 ms on C2,
// 0.322 -> 0.245 ms on a config-5 shard.  The weighted kernels (merged rows / EC counts) keep two.
__host__ __device__ constexpr int estep_batches(bool weighted, int ht) { return (weighted && ht <= 8) ? 2 : 1; }
// the mask's 0/1 doubles read from LDS nibble tables instead of built on the VALU (8 haplotypes, one batch at a time)
#ifndef GBRS_FTAB
#define GBRS_FTAB 1
#endif
// (with 16 haplotypes the kernel is already LDS-bound on its theta reads: the tables made it 35 % slower)
__host__ __device__ constexpr bool estep_uses_ftab(int ub, int ht) { return GBRS_FTAB && ub == 1 && ht == 8; }
// Round 3, the unweighted 8-haplotype kernel: a lane keeps the theta row of the locus it is on in registers and
// re-reads it from LDS only when it moves on to another locus (in stream order a lane stays on one locus for long
// stretches), so most words cost no theta read at all - 4 of the 8 ds_read_b128 per word are gone.  The 16 registers
// come from the pending set: a lane that leaves a locus sends its sums to LDS at once instead of parking them (with the
// LDS pipe no longer busy reading theta the atomics are cheap; with the reads in place the same change cost +23 %).
// 74 VGPRs, E-step on C2 0.098 -> 0.089 ms (profiles/r03_estep_experiments.txt).
// "Long stretches" held while a locus had hundreds of reads behind it.  Since the run-word folds a dictionary id has a few
// dozen words and a lane's share of a tile about 15 batches: on the bench sample 85 % of a wavefront's later batches have
// two or three lanes changing id, and the whole wavefront takes the miss path below for them.  The layout answers that, not
// this file: in the counted runs the rows of one id start at multiples of a stripe S (em_plan.h, em_take_stripes;
// tile_pad_kernel), so the lanes change in the same batches - a quarter of them at S = 4 (profiles/estep_stripes.txt).
#ifndef GBRS_THETA_REGS
#define GBRS_THETA_REGS 1
#endif
__host__ __device__ constexpr bool estep_theta_regs(int ub, int ht, bool det) { return GBRS_THETA_REGS && ub == 1 && ht == 8 && !det; }
// A tile's theta in LDS.  8 / 16 haplotypes: H/2 planes of (theta[2k], theta[2k+1]) pairs, one pair per locus and
// plane, so that the 16-byte reads of a 16-lane group fall on bank group (dictionary index mod 16): lanes on
// the same locus broadcast, and the handful of neighbouring loci a group spans never collide.  (Locus-major
// rows of 64 / 128 B collide whenever two indices agree mod 4 / mod 2: SQ_LDS_BANK_CONFLICT was 10.5 M of
// 33 M LDS cycles per launch on C2.)  Other haplotype counts keep locus-major rows.
#ifndef GBRS_THETA_PLANES
#define GBRS_THETA_PLANES 1
#endif
__host__ __device__ constexpr bool theta_planar(int ht) { return GBRS_THETA_PLANES && (ht == 8 || ht == 16); }
// the persistent-zero low halves of the mask doubles (GBRS_MASK_ZLO) pay only with two batches in hand
__host__ __device__ constexpr bool estep_uses_zlo(int ub) {
#if defined(GBRS_MASK_ZLO)
    return ub == 2;
#else
    return false;
#endif
}

__device__ __forceinline__ double wave_shr1(double x) {
    // lane i <- lane i-1, lane 0 <- 0.0   (DPP wave_shr:1, no LDS traffic)
    int lo = __double2loint(x), hi = __double2hiint(x);
    lo = __builtin_amdgcn_update_dpp(0, lo, 0x138, 0xf, 0xf, false);
    hi = __builtin_amdgcn_update_dpp(0, hi, 0x138, 0xf, 0xf, false);
    return __hiloint2double(hi, lo);
}

__device__ __forceinline__ double quad_swap_pairs(double x) {
    // lane i <- lane i ^ 1   (DPP quad_perm [1,0,3,2])
    int lo = __double2loint(x), hi = __double2hiint(x);
    lo = __builtin_amdgcn_update_dpp(0, lo, 0xB1, 0xf, 0xf, true);      // (every lane has a source: no old value to set up)
    hi = __builtin_amdgcn_update_dpp(0, hi, 0xB1, 0xf, 0xf, true);
    return __hiloint2double(hi, lo);
}

// Word bits that must be clear for the pair-swap row sum: a word fits when it is alone (pos = rem = 0), the first
// of two on an even lane (rem = 1) or the second of two on an odd lane (pos = 1), i.e. when its (rem | pos)
// field pair is 0 or exactly the one bit its lane allows.
__device__ __forceinline__ uint32_t pair_misfit_bits(int H, int PB, int lane) {
    const uint32_t pm = (1u << PB) - 1u;
    const uint32_t fields = (pm | (pm << PB)) << H;
    return fields & ~(((lane & 1) ? 1u : (1u << PB)) << H);
}

// 1.0 where bit h of mask is set, else 0.0, built from integer ops only
__device__ __forceinline__ double bit_as_double(uint32_t mask, int h) {
    const int m = __builtin_amdgcn_sbfe(mask, h, 1);             // 0 or -1  (v_bfe_u32 + v_cvt_f64_u32 measured slower)
    return __hiloint2double(m & 0x3FF00000, 0);
}

// Votes on a bool.  HIP's __any / __ballot take an int: hipcc 7.2 then materialises the predicate as 0/1 in a
// vector register and compares it again (two vector instructions per vote); these stay on the lane mask -
// as long as the bool is one comparison: an AND of two is voted on separately and combined as 64-bit words.
#ifndef GBRS_RECIP_GUARD_MAX
#define GBRS_RECIP_GUARD_MAX 1       // 1: v_max_f64 keeps a zero denominator finite; 0: compare + select of the high half
#endif
__device__ __forceinline__ uint64_t wave_ballot(bool p) { return __builtin_amdgcn_ballot_w64(p); }
__device__ __forceinline__ bool wave_any(bool p) { return __builtin_amdgcn_ballot_w64(p) != 0; }

__device__ __forceinline__ double fast_recip(double d) {
    // v_rcp_f64 seed + two Newton steps: <= 1 ulp for normal d > 0
    double r = __builtin_amdgcn_rcp(d);
    double e = fma(-d, r, 1.0);
    r = fma(r, e, r);
#if defined(GBRS_RECIP_ONE_NEWTON)
    return r;                     // experiment: one step (the seed's relative error squared)
#else
    e = fma(-d, r, 1.0);
    return fma(r, e, r);
#endif
}

// Per-lane accumulation state: the partial sums of the locus the lane is currently on (c), the
// ones of the locus it just left (pc, "pending"), and the float-error flag.
typedef double theta_pair_t __attribute__((ext_vector_type(2)));
template <int HC>
struct LaneAcc {
    double c[HC], pc[HC];
    // estep_theta_regs: theta of the lane's current locus (pc is then unused), as the 16-byte pairs the LDS reads deliver:
    // one register tuple per read wherever the value lives (kept as single doubles, the kernel with two batch loops held
    // the row twice - as tuples inside a loop, as doubles between the loops - and went to scratch)
    theta_pair_t th[(HC + 1) / 2];
    uint32_t cidx, pidx;
    uint64_t bad;      // lanes that met a row without abundance, as a wave-uniform ballot word: scalar ORs, no vector
                       // work (and an integer on purpose: as a loop-carried bool - an i1 lane mask - hipcc 7.2 mis-lowered it)
                       // when the loop gained an early exit (stale mask at the exit block: spurious float errors)
};

// Deterministic flush (GBRS_EM_DETERMINISTIC): the wavefront owns a private copy of the tile's sums, so
// no other wave touches it; inside the wave, the lanes that hand in sums for the same dictionary entry
// are added by a fixed butterfly tree (non-members contribute 0.0) and the entry's first lane applies the
// total with a plain read-modify-write.  Which lanes flush, and when, depends on the word stream only,
// so two launches add the same numbers in the same association: bit-identical sums.
template <int HC>
__device__ __forceinline__ void det_flush(double *__restrict__ wave_acc, int H, int lane, uint32_t &fidx,
                                          const double (&vals)[HC]) {
    unsigned long long todo = __ballot(fidx != 0xFFFFFFFFu);
    while (todo) {
        const int leader = __ffsll((long long)todo) - 1;
        const uint32_t idx = (uint32_t)__builtin_amdgcn_readlane((int)fidx, leader);
        const bool mine = fidx == idx;
        const unsigned long long grp = __ballot(mine);
        if (grp == (1ull << leader)) {
            // the usual case in stream order: one lane hands in this entry - nothing to order
            if (mine) {
#pragma unroll
                for (int h = 0; h < HC; ++h)
                    if (h < H) wave_acc[idx * H + h] += vals[h];
            }
        } else {
#pragma unroll
            for (int h = 0; h < HC; ++h) {
                if (h < H) {
                    const double tot = wave_sum_all(mine ? vals[h] : 0.0);
                    if (lane == leader) wave_acc[idx * H + h] += tot;
                }
            }
        }
        todo &= ~grp;
        if (mine) fidx = 0xFFFFFFFFu;
    }
}

// Two batches (UB = 2) of one wavefront: theta sums, row sums, reciprocals as independent chains,
// then the register accumulation in order.  w / wt: this lane's words (and per-word row weights).
template <bool WEIGHTED>
__device__ __forceinline__ void load_theta16(const double *__restrict__ s_theta, uint32_t idx, double (&t)[16]) {
    if (theta_planar(16)) {
        constexpr int DP = lds_theta_doubles(WEIGHTED, 16) / 16;
        const double2 *t2 = reinterpret_cast<const double2 *>(s_theta) + idx;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const double2 q = t2[k * DP];
            t[2 * k] = q.x;
            t[2 * k + 1] = q.y;
        }
    } else {
#pragma unroll
        for (int h = 0; h < 16; ++h) t[h] = s_theta[idx * 16 + h];
    }
}

// LEAD: a batch of the tile's leading run of one-word rows (TileHdr::n_one): no row sum, like ONEWORD; and in the kernel that
// keeps theta in registers the batch neither looks for padding words nor votes on a zero denominator:
//   * an empty cell of these batches has no haplotype bit and the dictionary index of the cell above it (em_layout.hip,
//     fill_one_word_cells_kernel), so it multiplies 0.0 into everything and hands nothing in; the cells of a lane that is
//     empty from the top are on entry 0 - one hand-in of nothing, and entry 0's theta row is a valid LDS row;
//   * a real row without abundance still divides the smallest normal number (the v_max_f64 guard) and so adds >= 4.49e307
//     to at least one of the tile's sums: the tile epilogue, which walks the sums anyway, raises the float error there.
template <int HT, bool WEIGHTED, int HC, bool DET, int UB, bool ONEWORD = false, bool LEAD = false>
__device__ __forceinline__ void tile_batches(const uint32_t (&w)[UB], const double (&wt)[UB], int H, int PB, int lane,
                                             const double *__restrict__ s_theta, double *__restrict__ my_acc,
                                             LaneAcc<HC> &st, const int (&zlo)[32], const double2 *__restrict__ s_ftab,
                                             uint32_t misfit_bits, uint32_t relax_zero_weight = 0u,
                                             int count_form = 0 /* general form: 1 a batch below TileHdr::n_one, 2 a batch of
                                                                   the counted two-word run behind it; wave-uniform */,
                                             bool pair = false /* LEAD form: a batch of the counted two-word run; wave-uniform */) {
    constexpr bool COUNTS = HT > 0 && HT <= 8 && !WEIGHTED && !DET && UB == 1;     // the instances that meet count fields
    constexpr bool PAIRS = COUNTS && !ONEWORD;                                     // ... and counted two-word runs
    constexpr bool ZLO = estep_uses_zlo(UB);
    constexpr bool FTAB = estep_uses_ftab(UB, HT);
    constexpr bool TREG = estep_theta_regs(UB, HT, DET) && HC >= 8;
    constexpr bool DIET = LEAD && TREG;
    const uint32_t hmask = (1u << H) - 1u, pmask = (1u << PB) - 1u;
    uint32_t mask[UB], idx[UB];
    int pos[UB], rem[UB];
    double s[UB];
    double f8[UB][8], f16[UB][16];          // HT == 8 / 16 with GBRS_MASK_ZLO: the words' 0/1 doubles
    (void)f8;
    (void)f16;
    // a counted batch's pos / rem bits are a repeat count (read where v is made): the row-length logic sees them cleared
    const uint32_t count_bits = (COUNTS && !LEAD && count_form != 0) ? ((1u << (2 * PB)) - 1u) << H : 0u;     // wave-uniform
#pragma unroll
    for (int u = 0; u < UB; ++u) {
        mask[u] = w[u] & hmask;
        pos[u] = ((w[u] & ~count_bits) >> H) & pmask;
        rem[u] = ((w[u] & ~count_bits) >> (H + PB)) & pmask;
        idx[u] = w[u] >> (H + 2 * PB);
    }
    uint64_t real_lanes0 = 0;                                    // TREG: lanes whose word is not padding
    (void)real_lanes0;
    if constexpr (TREG && !DIET) real_lanes0 = wave_ballot(mask[0] != 0);
    if constexpr (TREG) {
        // A lane that moves on to another locus hands the sums of the one it leaves to LDS (H atomics under the
        // branch's exec mask) and fetches the new locus's theta row, before the word's own arithmetic.
        const bool miss = DIET ? idx[0] != st.cidx : (mask[0] != 0) & (idx[0] != st.cidx);
        const uint64_t miss_lanes = DIET ? wave_ballot(idx[0] != st.cidx) : real_lanes0 & wave_ballot(idx[0] != st.cidx);
        if (miss_lanes != 0) {
            if (miss) {
                // (requesting the new locus's theta row - and the word's 0/1 doubles - before the old sums are handed in, so
                // that they do not arrive behind the eight float atomics, measured 2.5 % slower: profiles/r03_estep_experiments.txt item 7)
                if (st.cidx != 0xFFFFFFFFu) {
                    double *ap = my_acc + st.cidx * H;
#pragma unroll
                    for (int h = 0; h < HC; ++h)
                        if (h < H) atomicAdd(ap + h, st.c[h]);
                }
#pragma unroll
                for (int h = 0; h < HC; ++h) asm volatile("v_mov_b64 %0, 0" : "+v"(st.c[h]));     // in place, under the exec mask
                st.cidx = idx[0];
                constexpr int DPT = theta_planar(8) ? lds_theta_doubles(WEIGHTED, 8) / 8 : 1;
                const double2 *t2 = theta_planar(8) ? reinterpret_cast<const double2 *>(s_theta) + idx[0]
                                                    : reinterpret_cast<const double2 *>(s_theta + idx[0] * 8);
                const theta_pair_t *tv = reinterpret_cast<const theta_pair_t *>(t2);
                st.th[0] = tv[0]; st.th[1] = tv[DPT]; st.th[2] = tv[2 * DPT]; st.th[3] = tv[3 * DPT];
            }
        }
    }
#pragma unroll
    for (int u = 0; u < UB; ++u) {
        const double *tp = s_theta + idx[u] * H;
        double su = 0.0;
#if defined(GBRS_ABLATE_THETA)
        su = __hiloint2double(0x3FF00000 | (mask[u] << 4), idx[u]);
        if (false) {
#else
        if (HT == 8) {
#endif
            constexpr int DP = theta_planar(8) ? lds_theta_doubles(WEIGHTED, 8) / 8 : 1;      // pairs per plane
            const double2 *t2 = theta_planar(8) ? reinterpret_cast<const double2 *>(s_theta) + idx[u]
                                                : reinterpret_cast<const double2 *>(tp);      // 64-byte aligned row
            const double2 a = TREG ? make_double2(st.th[0].x, st.th[0].y) : t2[0], cc = TREG ? make_double2(st.th[1].x, st.th[1].y) : t2[DP],
                          e = TREG ? make_double2(st.th[2].x, st.th[2].y) : t2[2 * DP], g = TREG ? make_double2(st.th[3].x, st.th[3].y) : t2[3 * DP];
            // two chains of four to halve the dependent-FMA latency
            double s0, s1;
            if constexpr (FTAB) {
                // the mask's 0/1 doubles from two 16-entry LDS tables indexed by a nibble of the mask (pairs
                // (f0,f1) and (f2,f3) of the nibble; each table is 256 B = one pass over the 64 banks, so the
                // four 16-byte reads are conflict free): no vector instruction is spent on building them
                const uint32_t lo = mask[u] & 15u, hi = mask[u] >> 4;
                const double2 p0 = s_ftab[lo], p1 = s_ftab[16 + lo], p2 = s_ftab[hi], p3 = s_ftab[16 + hi];
                f8[u][0] = p0.x; f8[u][1] = p0.y; f8[u][2] = p1.x; f8[u][3] = p1.y;
                f8[u][4] = p2.x; f8[u][5] = p2.y; f8[u][6] = p3.x; f8[u][7] = p3.y;
                s0 = f8[u][0] * a.x, s1 = f8[u][1] * a.y;
                s0 = fma(f8[u][2], cc.x, s0);
                s1 = fma(f8[u][3], cc.y, s1);
                s0 = fma(f8[u][4], e.x, s0);
                s1 = fma(f8[u][5], e.y, s1);
                s0 = fma(f8[u][6], g.x, s0);
                s1 = fma(f8[u][7], g.y, s1);
            } else if constexpr (ZLO) {
                // 0/1 doubles whose low halves are the caller's loop-invariant zero registers: only the
                // high half is rewritten per word (a fresh double costs a v_mov for its low half)
#pragma unroll
                for (int h = 0; h < 8; ++h)
                    f8[u][h] = __hiloint2double(__builtin_amdgcn_sbfe(mask[u], h, 1) & 0x3FF00000, zlo[u * 8 + h]);
                s0 = f8[u][0] * a.x, s1 = f8[u][1] * a.y;
                s0 = fma(f8[u][2], cc.x, s0);
                s1 = fma(f8[u][3], cc.y, s1);
                s0 = fma(f8[u][4], e.x, s0);
                s1 = fma(f8[u][5], e.y, s1);
                s0 = fma(f8[u][6], g.x, s0);
                s1 = fma(f8[u][7], g.y, s1);
            } else {
                s0 = bit_as_double(mask[u], 0) * a.x, s1 = bit_as_double(mask[u], 1) * a.y;
                s0 = fma(bit_as_double(mask[u], 2), cc.x, s0);
                s1 = fma(bit_as_double(mask[u], 3), cc.y, s1);
                s0 = fma(bit_as_double(mask[u], 4), e.x, s0);
                s1 = fma(bit_as_double(mask[u], 5), e.y, s1);
                s0 = fma(bit_as_double(mask[u], 6), g.x, s0);
                s1 = fma(bit_as_double(mask[u], 7), g.y, s1);
            }
            su = s0 + s1;
        } else if (ZLO && HT == 16) {
            double t16[16];
            load_theta16<WEIGHTED>(s_theta, idx[u], t16);
#pragma unroll
            for (int h = 0; h < 16; ++h) {
                f16[u][h] = __hiloint2double(__builtin_amdgcn_sbfe(mask[u], h, 1) & 0x3FF00000, zlo[u * 16 + h]);
                su = fma(f16[u][h], t16[h], su);
            }
        } else if (HT == 16) {
            double t16[16];
            load_theta16<WEIGHTED>(s_theta, idx[u], t16);
#pragma unroll
            for (int h = 0; h < 16; ++h) su = fma(bit_as_double(mask[u], h), t16[h], su);
        } else if (HT > 0) {
#pragma unroll
            for (int h = 0; h < HT; ++h) su = fma(bit_as_double(mask[u], h), tp[h], su);
        } else {
            for (int h = 0; h < H; ++h) su = fma(bit_as_double(mask[u], h), tp[h], su);
        }
        s[u] = su;
    }
    // den = sum of s over the words of my row.  Batches made of one-word rows only (very common:
    // the reads of one locus list are contiguous) need no cross-lane work at all.
    double den[UB];
    // (pos and rem are adjacent bit fields of the word: one AND finds a row of more than one word)
    const uint32_t fields = (pmask | (pmask << PB)) << H;
    const uint32_t multi = (UB == 1 ? w[0] : (w[0] | w[UB - 1])) & fields & ~count_bits;
    if (PAIRS && (LEAD ? pair : count_form == 2)) {
        // a counted batch of two-word rows: every lane's row total is its s plus its partner's, padding pairs included
        // (0 + 0, which the reciprocal's guard keeps finite and the 0.0 factors of the clear haplotype bits erase)
#pragma unroll
        for (int u = 0; u < UB; ++u) den[u] = s[u] + quad_swap_pairs(s[u]);
    } else
#if defined(GBRS_ABLATE_ROWSUM)
    if (true) {
#else
    if (ONEWORD || LEAD || !wave_any(multi != 0)) {       // ONEWORD: the layout holds no row of more than one word at all
#endif
#pragma unroll
        for (int u = 0; u < UB; ++u) den[u] = s[u];
    } else if (!wave_any((multi & misfit_bits) != 0)) {
        // nothing longer than two words, and every two-word row sits on an (even, odd) lane pair (stream
        // order puts them there): the row total is my s plus my partner's - one DPP swap inside the quad
#pragma unroll
        for (int u = 0; u < UB; ++u) {
            const double other = quad_swap_pairs(s[u]);
            den[u] = s[u] + (((w[u] & fields & ~count_bits) != 0) ? other : 0.0);
        }
    } else {
        // running sum over the pos words to my left ...
        double acc[UB], t[UB];
#pragma unroll
        for (int u = 0; u < UB; ++u) acc[u] = t[u] = s[u];
        const int pmax = max(pos[0], pos[UB - 1]);
        for (int d = 1; wave_any(pmax >= d); ++d) {
#pragma unroll
            for (int u = 0; u < UB; ++u) {
                t[u] = wave_shr1(t[u]);
                acc[u] += (pos[u] >= d) ? t[u] : 0.0;
            }
        }
        // ... whose value at the row's last word is the row total
#pragma unroll
        for (int u = 0; u < UB; ++u) den[u] = __shfl(acc[u], lane + rem[u], WAVE);
    }
    double v[UB];
#pragma unroll
    for (int u = 0; u < UB; ++u) {
        const bool ok = den[u] > 0.0;
        double r;
        // resampling handles (GBRS_EM_RESAMPLE, a wave-uniform kernel argument): a row whose weight is 0 takes no part, so a
        // zero denominator of its own is no float error; its words still add 0.0 * (a finite reciprocal)
        uint64_t counted = ~0ull;
        if constexpr (WEIGHTED) {
            if (relax_zero_weight) counted = wave_ballot(wt[u] != 0.0);
        }
        if constexpr (GBRS_RECIP_GUARD_MAX && TREG) {
            // padding words (no haplotype bit: den 0) and rows without abundance (flagged here, the step's result is then
            // discarded) divide the smallest normal number instead - one v_max_f64 keeps 1/den finite, and a padding
            // word's 0.0 factors turn it into nothing; the real-word lanes are the ballot taken at the top of the batch.
            // (Only in the kernel that has registers to spare: the 16-haplotype form spills with it.)
            if constexpr (!DIET) st.bad |= real_lanes0 & wave_ballot(!ok) & counted;      // (DIET: the tile epilogue finds it in the sums)
            double dsafe;
            asm("v_max_f64 %0, %1, %2" : "=v"(dsafe) : "v"(den[u]), "s"(2.2250738585072014e-308));   // (scalar operand: no registers)
            r = fast_recip(dsafe);
        } else {
            st.bad |= wave_ballot(mask[u] != 0) & wave_ballot(!ok) & counted;
            // padding words (no haplotype bit: den 0) and rows without abundance (flagged above, the step's result
            // is then discarded) divide a value in [1, 2) instead: one select on the high half keeps 1/den
            // finite, and a padding word's 0.0 factors turn it into nothing
            r = fast_recip(__hiloint2double(ok ? __double2hiint(den[u]) : 0x3FF00000, __double2loint(den[u])));
        }
        if (WEIGHTED) r *= wt[u];
        if constexpr (COUNTS) {
            // the word and the further reads it stands for: one field extract, one convert, one FMA - the same arithmetic in
            // both forms (a general-form batch past n_one skips it: its fields are positions)
            if (LEAD || count_form != 0) r = fma(r, (double)((w[u] >> H) & ((1u << (2 * PB)) - 1u)), r);
        }
        v[u] = r;
    }
#pragma unroll
    for (int u = 0; u < UB; ++u) {
        const bool miss = !TREG && (mask[u] != 0) & (idx[u] != st.cidx);
        const uint64_t miss_lanes = TREG ? 0 : wave_ballot(mask[u] != 0) & wave_ballot(idx[u] != st.cidx);
#if !defined(GBRS_ABLATE_ATOMICS)
        if (miss_lanes != 0) {
            // A lane that moves on to another locus parks its sums in the pending set; the LDS
            // atomics are only issued when some lane needs that set again, and then by every lane
            // that has something parked: one group of H wave-wide atomics per locus boundary.
            if (DET) {
                if ((miss_lanes & wave_ballot(st.pidx != 0xFFFFFFFFu)) != 0) det_flush<HC>(my_acc, H, lane, st.pidx, st.pc);
            } else if ((miss_lanes & wave_ballot(st.pidx != 0xFFFFFFFFu)) != 0) {
                if (st.pidx != 0xFFFFFFFFu) {
                    double *ap = my_acc + st.pidx * H;
#pragma unroll
                    for (int h = 0; h < HC; ++h)
                        if (h < H) atomicAdd(ap + h, st.pc[h]);
                    st.pidx = 0xFFFFFFFFu;
                }
            }
            if (miss) {
#pragma unroll
                for (int h = 0; h < HC; ++h) {
                    // two moves per haplotype, in place under the branch's exec mask (written as plain
                    // assignments the merge with the not-taken side costs a third copy per double)
                    asm volatile("v_mov_b64 %0, %1" : "+v"(st.pc[h]) : "v"(st.c[h]));
                    asm volatile("v_mov_b64 %0, 0" : "+v"(st.c[h]));
                }
                st.pidx = st.cidx;
                st.cidx = idx[u];
            }
        }
#else
        if (miss) st.cidx = idx[u];
#endif
        if (HT > 0) {
#pragma unroll
            for (int h = 0; h < HT; ++h) {
                if ((ZLO || FTAB) && HT == 8) { st.c[h] = fma(f8[u][h & 7], v[u], st.c[h]); continue; }
                if (ZLO && HT == 16) { st.c[h] = fma(f16[u][h & 15], v[u], st.c[h]); continue; }
                st.c[h] = fma(bit_as_double(mask[u], h), v[u], st.c[h]);
            }
        } else {
#pragma unroll
            for (int h = 0; h < HC; ++h)
                if (h < H) st.c[h] = fma(bit_as_double(mask[u], h), v[u], st.c[h]);
        }
    }
}

// Sum of the K privatised copies of one element of a tile's sums (K a power of two, 1..64), copies added in index order in
// groups of eight whose LDS reads are all in flight together: a one-locus tile has 64 copies of its 8 elements, and eight
// threads that each walk 64 dependent reads cost the workgroup ~4 us at the end of the tile (scripts/tile_timeline_persistent.py).
template <bool ZERO>
__device__ __forceinline__ double sum_copies(double *__restrict__ s_acc, uint32_t i, uint32_t K, uint32_t stride) {
    double a = 0.0;
    if (K >= 8) {
        for (uint32_t c = 0; c < K; c += 8) {
            double v[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) v[q] = s_acc[(c + q) * stride + i];
            if (ZERO) {
#pragma unroll
                for (int q = 0; q < 8; ++q) s_acc[(c + q) * stride + i] = 0.0;
            }
#pragma unroll
            for (int q = 0; q < 8; ++q) a += v[q];
        }
    } else {
        double v[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) v[q] = s_acc[min((uint32_t)q, K - 1u) * stride + i];
        if (ZERO) {
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if ((uint32_t)q < K) s_acc[q * stride + i] = 0.0;
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) a += (uint32_t)q < K ? v[q] : 0.0;
    }
    return a;
}

#if defined(GBRS_DIAG_TILE_TIMES)
// Diagnostic build only (scripts/tile_timeline.py): every tile of the EM step's E-step launch records when it started,
// entered and left its batch loop and ended (s_memrealtime, 100 MHz) and where it ran (HW_ID / XCC_ID).
__device__ unsigned long long *g_tile_stamps = nullptr;
__device__ __forceinline__ void diag_stamp(int slot, unsigned long long extra = 0) {
    if (g_tile_stamps && threadIdx.x == 0) {
        g_tile_stamps[(size_t)blockIdx.x * 8 + slot] = __builtin_amdgcn_s_memrealtime();
        if (slot == 0) {
            g_tile_stamps[(size_t)blockIdx.x * 8 + 4] = __builtin_amdgcn_s_getreg((31 << 11) | (0 << 6) | 4);    // HW_ID, 32 bits
            g_tile_stamps[(size_t)blockIdx.x * 8 + 5] = __builtin_amdgcn_s_getreg((3 << 11) | (0 << 6) | 20);   // XCC_ID, 4 bits
            g_tile_stamps[(size_t)blockIdx.x * 8 + 5] |= extra << 8;
        }
    }
}
#define GBRS_DIAG_STAMP(...) do { if (!ONES) diag_stamp(__VA_ARGS__); } while (0)
// persistent kernel (scripts/tile_timeline_persistent.py): the record of TILE t, written by thread 0 of the workgroup that has it
#define GBRS_DIAG_PSTAMP(t, slot) do { if (g_tile_stamps && threadIdx.x == 0) g_tile_stamps[(size_t)(t) * 8 + (slot)] = __builtin_amdgcn_s_memrealtime(); } while (0)
#else
#define GBRS_DIAG_STAMP(...) do { } while (0)
#define GBRS_DIAG_PSTAMP(t, slot) do { } while (0)
#endif

// ---- the gather-side M-step (em_layout.h, GatherArgs) -----------------------------------------------------------------
// One (slot, member) of a tile's dictionary at haplotype h: theta, A of the iteration before and the length are loaded
// together (gm_load), then theta' = theta * A / len - the arithmetic and order of mstep_row (em_mstep.inc) - is what the tile
// puts into LDS.  The owner's H adjacent lanes store theta', the locus's totals (locus_total's pairing tree, one haplotype
// per lane: xor 1, 2, 4) and add to the tile's block sums; they zero the locus's row of the A vector the next launch adds
// into.  Without `pending` theta is current and only the zeroing is stored.
struct GatherMember { double t, a, ln; };
template <int H>
__device__ __forceinline__ GatherMember gm_load(const GatherArgs &ga, const double *__restrict__ theta, uint32_t g, uint32_t h) {
    const size_t i = (size_t)(g & GSLOT_LOCUS) * H + h;
    GatherMember m;
    m.t = theta[i];
    m.a = ga.acc_old[i];
    m.ln = ga.eff_len ? ga.eff_len[i] : 1.0;
    return m;
}
// locus_total's tree (em_mstep.inc) over one haplotype per lane.  locus_total asks for every lane of the wavefront active;
// here the calls sit in divergent code (the prologue's loop tail, the branches on the kind of entry), which is fine because a
// DPP step only reads lanes of the locus's own group of H: element i = j * H + h of the dictionary goes to thread i mod
// TILE_THREADS, H divides 64, so the H lanes of an entry are an aligned group, take every branch together (the branches test
// the entry, not the haplotype) and are active or inactive as one.
template <int H>
__device__ __forceinline__ double gm_total(double x) {
    if (H >= 2) x += mstep_dpp<0xB1>(x);         // quad_perm:[1,0,3,2]
    if (H >= 4) x += mstep_dpp<0x4E>(x);         // quad_perm:[2,3,0,1]
    if (H >= 8) x += mstep_dpp<0x141>(x);        // row_half_mirror
    return x;
}
template <int H>
__device__ __forceinline__ double gm_apply(const GatherArgs &ga, uint32_t g, uint32_t h, const GatherMember &m, bool live,
                                           double &sum_old, double &sum_new) {
    const uint32_t l = g & GSLOT_LOCUS;
    const size_t i = (size_t)l * H + h;
    const bool owner = (g & GSLOT_OWNER) != 0 && live;
    double tn = m.t;
    if (ga.pending) {                            // (a kernel argument: uniform)
        const double c = m.t * m.a;
        tn = c / m.ln;                           // (no lengths: c / 1.0 is c)
        const double tp = gm_total<H>(m.t), tq = gm_total<H>(tn);
        if (owner) {
            ga.theta_new[i] = tn;
            if (h == 0) {
                ga.tot_prev[l] = tp;
                ga.tot_new[l] = tq;
            }
            sum_old += m.t;
            sum_new += tn;
        }
    }
    if (owner && !(g & GSLOT_DIRECT)) ga.acc_next[i] = 0.0;
    return tn;
}

// The tile prologue of the gather-side route: the same dependent trips as the plain gather (header -> dictionary -> theta),
// A and the length fetched in the last one.  A two-member set does both members and stores their sum, a larger set its
// members in member order.  The tile's two block sums go to one slot per wavefront (fixed order, no atomics).
template <int H, bool WEIGHTED>
__device__ __forceinline__ void tile_gather_prologue(const TileHdr &th, uint32_t DH, const uint32_t *__restrict__ dict,
                                                     const uint32_t *__restrict__ slot_dest, const double *__restrict__ theta,
                                                     const SetArgs &sets, const GatherArgs &ga, bool live, int wave,
                                                     double *__restrict__ s_theta) {
    double sum_old = 0.0, sum_new = 0.0;
    for (uint32_t i = threadIdx.x; i < DH; i += TILE_THREADS) {
        const uint32_t j = i / H, h = i - j * H, p = th.dict_base + j;
        const uint32_t e = dict[p], g = ga.gdest[p];
        double tv;
        if (sets.set_ptr == nullptr || !(e & (DICT_PAIR | DICT_SET))) {
            tv = gm_apply<H>(ga, g, h, gm_load<H>(ga, theta, g, h), live, sum_old, sum_new);
        } else if (e & DICT_PAIR) {
            const uint32_t g2 = ga.gdest_b[p];
            const GatherMember m0 = gm_load<H>(ga, theta, g, h), m1 = gm_load<H>(ga, theta, g2, h);
            const double t0 = gm_apply<H>(ga, g, h, m0, live, sum_old, sum_new);
            const double t1 = gm_apply<H>(ga, g2, h, m1, live, sum_old, sum_new);
            tv = t0 + t1;
        } else {
            const uint32_t *gl = ga.gdest_list + (slot_dest[p] & ~SLOT_SET);
            const uint32_t n = gl[0];
            tv = 0.0;
            for (uint32_t q = 1; q <= n; ++q) {
                const uint32_t gq = gl[q];
                tv += gm_apply<H>(ga, gq, h, gm_load<H>(ga, theta, gq, h), live, sum_old, sum_new);
            }
        }
        constexpr uint32_t DP = theta_planar(H) ? lds_theta_doubles(WEIGHTED, H) / H : 0;
        s_theta[theta_planar(H) ? (((h >> 1) * DP + j) << 1) + (h & 1u) : i] = tv;
    }
    if (ga.pending) {
        sum_old = wave_sum_all(sum_old);
        sum_new = wave_sum_all(sum_new);
        if ((threadIdx.x & 63) == 0 && live) {
            ga.msums[(size_t)blockIdx.x * TILE_WAVES + wave] = sum_old;
            ga.msums[(size_t)ga.cap + (size_t)blockIdx.x * TILE_WAVES + wave] = sum_new;
        }
    }
}

template <int HT, bool WEIGHTED, bool ONES, bool DET = false, bool ONEWORD = false, bool GATHER = false>
// (the deterministic 8-haplotype form spills 12-16 B per lane at 6 waves per SIMD - 80 registers + its flush tree.  Compiled
// for 4 waves it needs 84 registers and no scratch, and is SLOWER: 0.949 against 0.82 ms per iteration on C2 (round 4) - the
// spill sits in the rare ordered-flush path, the occupancy pays on every batch.  So the scratch stays.)
#if defined(GBRS_ESTEP_VGPR_CAP)
__attribute__((amdgpu_num_vgpr(GBRS_ESTEP_VGPR_CAP)))      // experiment: 8 waves per SIMD need <= 64 registers
#endif
__global__ void __launch_bounds__(TILE_THREADS, (HT > 0 && HT <= 8) ? (WEIGHTED ? 4 : GBRS_ESTEP_WAVES) : (WEIGHTED ? 3 : GBRS_ESTEP_WAVES16))   // 4 = two workgroups per CU
tile_estep_kernel(uint32_t Hrt, const TileHdr *__restrict__ tiles, const uint32_t *__restrict__ words,
                  const uint32_t *__restrict__ dict, const double *__restrict__ word_weight,
                  const double *__restrict__ theta, double *__restrict__ partials,
                  const uint32_t *__restrict__ slot_dest, double *__restrict__ acc_direct,
                  EmScalars *__restrict__ sc, uint32_t n_tiles, ErrArgs ea, SetArgs sets,
                  uint32_t lead_mask /* ~0: the headers' n_one is used; 0: one loop for every batch */,
                  GatherArgs ga /* GATHER: the M-step of the iteration before rides the prologue; else not read */) {
    static_assert(!GATHER || (HT > 0 && HT <= 8 && !WEIGHTED && !ONES && !DET), "the gather-side M-step: unweighted, 1-8 haplotypes");
    constexpr int LDS_ACC_DOUBLES = lds_acc_doubles(WEIGHTED, HT);
    __shared__ __attribute__((aligned(16))) double s_theta[lds_theta_doubles(WEIGHTED, HT)];
    __shared__ __attribute__((aligned(16))) double2 s_ftab[32];      // [16] pairs (bit0, bit1) of a nibble, [16] pairs (bit2, bit3)
    if (estep_uses_ftab(estep_batches(WEIGHTED, HT), HT) && threadIdx.x < 32) {
        const uint32_t k = threadIdx.x & 15u, sh = (threadIdx.x >> 4) * 2;
        s_ftab[threadIdx.x] = make_double2((double)((k >> sh) & 1u), (double)((k >> (sh + 1)) & 1u));
    }
    __shared__ __attribute__((aligned(16))) double s_acc[LDS_ACC_DOUBLES];
    __shared__ uint32_t s_stop;
    // workgroups past the tiles run the previous step's deferred error pass (em.hip, em_finish_step):
    // it does not feed this E-step, it only has to finish before the next M-step
    if (blockIdx.x >= n_tiles) {
        if (!ONES) err_finish_body(ea, blockIdx.x - n_tiles);
        return;
    }
    // the stop flag's load is issued here and looked at after the tile header and the first words are on their way
    const uint32_t stop_flag = ONES ? 0u : sc->stop;
    const int H = HT > 0 ? HT : (int)Hrt;
    const int PB = pos_bits(H);
#if defined(GBRS_ESTEP_PRIO)                     // experiment: the tile's prologue and epilogue ahead of other tiles' batch loops
    __builtin_amdgcn_s_setprio(GBRS_ESTEP_PRIO);
#endif
    const TileHdr th = tiles[blockIdx.x];
    GBRS_DIAG_STAMP(0, th.n_batches);
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    // Each wavefront takes a contiguous run of the tile's batches, so a lane meets the same locus
    // again 64 words later and keeps its partial sums in registers (LaneAcc).  The E-step is a
    // pure stream of words: to cover HBM latency every wavefront keeps PD batches (2 KiB) in
    // flight, starting before the tile prologue (4 in the weighted form, whose second ring of
    // per-word weights otherwise pushes the kernel into scratch).
#ifndef GBRS_WEIGHTED_PD
#define GBRS_WEIGHTED_PD 4
#endif
#ifndef GBRS_RAW_PD
#define GBRS_RAW_PD 4
#endif
#ifndef GBRS_H16_PD
#define GBRS_H16_PD 8
#endif
    constexpr int UB = estep_batches(WEIGHTED, HT), PD = WEIGHTED ? GBRS_WEIGHTED_PD : (HT == 16 ? GBRS_H16_PD : GBRS_RAW_PD);
    const uint32_t b0 = (uint32_t)(((uint64_t)th.n_batches * wave) / TILE_WAVES);
    const uint32_t b1 = (uint32_t)(((uint64_t)th.n_batches * (wave + 1)) / TILE_WAVES);
    // Two loops over this wavefront's batches: the whole rings of it that lie in the tile's leading one-word batches
    // (TileHdr::n_one) through the LEAD form of tile_batches, the rest through the general one.  What the general form asks of
    // every batch - is any row longer than a word, is this word padding, is a denominator zero - the layout has answered for
    // those batches once.  The switch falls on a ring boundary; the lanes' state carries over, and the arithmetic and
    // its association are the single loop's.
    constexpr bool SPLIT = HT > 0 && HT <= 8 && !WEIGHTED && !DET;
    // The counted run of two-word rows behind them (TileHdr::n_two) goes through the same first loop: a batch at or past
    // n_one takes the pair form of the row sum under a wave-uniform scalar, so a ring that holds the last one-word batches
    // and the first two-word ones needs no loop of its own (three copies of the batch loop - one-word, pair, general -
    // would leave that ring, and the registers of a third copy, to the general form).
    const uint32_t n_one = SPLIT ? (uint32_t)th.n_one : 0u;
    const uint32_t n_lead = SPLIT ? ((n_one + (ONEWORD ? 0u : th.n_two())) & lead_mask) : 0u;
    uint32_t bm = b0;
    if (SPLIT && n_lead > b0) bm = b0 + ((min(b1, n_lead) - b0) / PD) * PD;
    // The ring is filled through a buffer descriptor of this wavefront's run [tile base, batch b1): the address is
    // one 32-bit vector offset advanced once per PD batches (the slot is an immediate), and a batch past the
    // run reads as zero words through the descriptor's range check - no branch, no select.
    const uint32_t *wp = words + (size_t)th.batch_base * 64;
    const double *wtp = WEIGHTED ? word_weight + (size_t)th.batch_base * 64 : nullptr;
    const __amdgpu_buffer_rsrc_t wres = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint32_t *>(wp), 0, (int)(b1 * 256u), 0x00020000);
    const __amdgpu_buffer_rsrc_t wtres = __builtin_amdgcn_make_buffer_rsrc(const_cast<double *>(WEIGHTED ? wtp : (const double *)wp), 0,
                                                                          WEIGHTED ? (int)(b1 * 512u) : 0, 0x00020000);
    int voff = (int)(b0 * 256u) + lane * 4;              // of batch b, advanced with it
    auto load_word = [&](int ahead) -> uint32_t {        // my word of batch b + ahead
        return (uint32_t)__builtin_amdgcn_raw_buffer_load_b32(wres, voff + ahead * 256, 0, 0);
    };
    auto load_weight = [&](int ahead) -> double {
        const auto q = __builtin_amdgcn_raw_buffer_load_b64(wtres, 2 * voff + ahead * 512, 0, 0);
        return __hiloint2double((int)q[1], (int)q[0]);
    };
    uint32_t ring[PD];
    double wring[WEIGHTED ? PD : 1];
#pragma unroll
    for (int u = 0; u < PD; ++u) {
        ring[u] = load_word(u);
        if (WEIGHTED) wring[u] = load_weight(u);
    }
    const uint32_t DH = th.template dict_count_of<SPLIT>() * H;
    const uint32_t stride = DH | 1u;                       // odd: copies fall on different banks
    uint32_t K = LDS_ACC_DOUBLES / stride;
    K = K >= 64 ? 64u : (1u << (31 - __clz((int)K)));       // power of two, 1..64
    // theta of the tile's dictionary: two dependent loads per element (dictionary entry, then theta of that locus), a plain
    // loop.  Issuing all of a thread's dictionary loads, then all its theta loads, then the LDS stores (and the same for the
    // epilogue's destinations) shortens a tile's prologue but measured 2.5 % SLOWER per launch (0.0897 vs 0.0872 ms, same
    // box, profiles/r03_estep_experiments.txt item 5): the other two workgroups of the CU fill the wait, and the
    // bursts compete with their word stream.
#if defined(GBRS_ABLATE_PROLOGUE)
    constexpr bool gather_ones = true;
#else
    constexpr bool gather_ones = ONES;
#endif
    for (uint32_t i = threadIdx.x; i < K * stride; i += TILE_THREADS) s_acc[i] = 0.0;
    GBRS_DIAG_STAMP(7);
    // (GATHER: a stopped launch stores nothing at all - the flag is waited for in front of the prologue's first store)
    if constexpr (GATHER) tile_gather_prologue<HT, WEIGHTED>(th, DH, dict, slot_dest, theta, sets, ga, stop_flag == 0, wave, s_theta);
    else
    for (uint32_t i = threadIdx.x; i < DH; i += TILE_THREADS) {
        const uint32_t j = i / H, h = i - j * H;
        constexpr uint32_t DP = theta_planar(HT) ? lds_theta_doubles(WEIGHTED, HT) / (HT > 0 ? HT : 1) : 0;
        const uint32_t at = theta_planar(HT) ? (((h >> 1) * DP + j) << 1) + (h & 1u) : i;
        double tv;
#if defined(GBRS_ABLATE_PROLOGUE_FULL)
        if (true) {
            tv = 1.0;
        } else
#endif
        if (sets.set_ptr == nullptr) {
            tv = gather_ones ? 1.0 : theta[(size_t)dict[th.dict_base + j] * H + h];
        } else {
            // a dictionary entry may be a locus set (em_layout.h): its theta is the sum of its members', in member order.
            // A two-member set has both members in the dictionary itself (entry and dict_b, fetched together): the same
            // two round trips as a locus; a larger set goes through its member list.
            const uint32_t e = dict[th.dict_base + j], e2 = sets.dict_b[th.dict_base + j];
            if (!(e & (DICT_PAIR | DICT_SET))) {
                tv = gather_ones ? 1.0 : theta[(size_t)e * H + h];
            } else if (e & DICT_PAIR) {
                if (gather_ones) {
                    tv = 2.0;
                } else {
                    const double t0 = theta[(size_t)(e & ~DICT_PAIR) * H + h], t1 = theta[(size_t)e2 * H + h];
                    tv = t0 + t1;
                }
            } else {
                const uint32_t k = e & ~DICT_SET;
                const uint32_t m0 = sets.set_ptr[k], m1 = sets.set_ptr[k + 1];
                tv = 0.0;
                if (gather_ones) {
                    tv = (double)(m1 - m0);
                } else {
                    // SETB members at a time: their ids together, then their theta together (clamped, not predicated:
                    // a branch around a load puts a wait behind it).  (One at a time in the unweighted 16-haplotype
                    // kernel, which sits at its 128-register budget and spills otherwise.)
                    constexpr int SETB = (HT == 16 && !WEIGHTED) ? 1 : 4;
                    for (uint32_t m = m0; m < m1; m += SETB) {
                        uint32_t mem[SETB];
                        double tm[SETB];
#pragma unroll
                        for (int q = 0; q < SETB; ++q) mem[q] = sets.set_members[min(m + q, m1 - 1)];
#pragma unroll
                        for (int q = 0; q < SETB; ++q) tm[q] = theta[(size_t)mem[q] * H + h];
#pragma unroll
                        for (int q = 0; q < SETB; ++q) tv += m + q < m1 ? tm[q] : 0.0;
                    }
                }
            }
        }
        s_theta[at] = tv;
    }
    // (the stop flag is looked at here, not before the gather: its round trip then runs beside the gather's, and a
    // stopped launch has read a little theta for nothing - it stores nothing)
    GBRS_DIAG_STAMP(6);
    // One verdict per workgroup: in pair mode (gbrs_em_pair_check) the partner's error pass may raise the flag while this
    // launch is running, and wavefronts that read it on their own could part ways around the barriers below.
    if (threadIdx.x == 0) s_stop = stop_flag;
    __syncthreads();
    if (s_stop) return;
    GBRS_DIAG_STAMP(1);
#if defined(GBRS_ESTEP_PRIO)
    __builtin_amdgcn_s_setprio(0);
#endif
    // default: lanes spread over the K copies; deterministic: one copy per wavefront (the layout was cut
    // with at most det_dict_cap(H) loci per tile, so K >= TILE_WAVES)
    double *my_acc = s_acc + (DET ? (uint32_t)wave : (lane & (K - 1))) * stride;
    constexpr int HC = HT > 0 ? HT : 16;
    int zlo[32];                            // opaque zeros: see GBRS_MASK_ZLO in tile_batches
#pragma unroll
    for (int k = 0; k < 32; ++k) {
        if constexpr (estep_uses_zlo(estep_batches(WEIGHTED, HT))) asm volatile("v_mov_b32 %0, 0" : "=v"(zlo[k]));
        else zlo[k] = 0;
    }
    LaneAcc<HC> st;
#pragma unroll
    for (int h = 0; h < HC; ++h) st.c[h] = st.pc[h] = 0.0;
    if constexpr (estep_theta_regs(UB, HT, DET)) {
#pragma unroll
        for (int h = 0; h < HC / 2; ++h) st.th[h] = theta_pair_t{0.0, 0.0};       // finite: a padding word multiplies it by 0.0
    }
    st.cidx = st.pidx = 0xFFFFFFFFu;
    st.bad = 0;
    if constexpr (SPLIT) {
        for (uint32_t b = b0; b < bm; b += PD) {
#pragma unroll
            for (int tt = 0; tt < PD; ++tt) {
                const uint32_t w[1] = {ring[tt]};
                const double wt[1] = {1.0};
                ring[tt] = load_word(PD + tt);                         // refill PD batches ahead
                tile_batches<HT, false, HC, false, 1, ONEWORD, true>(w, wt, H, PB, lane, s_theta, my_acc, st, zlo, s_ftab, 0u, 0u, 0,
                                                                     !ONEWORD && b + tt >= n_one);
            }
            voff += PD * 256;
            asm volatile("" : "+v"(voff));
        }
        if constexpr (estep_theta_regs(UB, HT, DET)) {
            // (opaque: the theta registers of the two loops are then one set inside each loop, not a pair of them)
#pragma unroll
            for (int h = 0; h < HC / 2; ++h) asm volatile("" : "+v"(st.th[h]));
        }
    }
    // (what only the general form needs is made here, behind the first loop, from an opaque copy of the lane: it is not
    // carried in a register through that loop)
    int lane_g = lane;
    if constexpr (SPLIT) asm volatile("" : "+v"(lane_g));
    const uint32_t misfit_bits = pair_misfit_bits(H, PB, lane_g);
#if defined(GBRS_ABLATE_BATCHES)
    for (uint32_t b = bm; b < bm; b += PD) {
#else
    for (uint32_t b = bm; b < b1; b += PD) {
#endif
#pragma unroll
        for (int tt = 0; tt < PD / UB; ++tt) {
            uint32_t w[UB];
            double wt[UB];
#pragma unroll
            for (int u = 0; u < UB; ++u) {
                const int slot = tt * UB + u;
                w[u] = ring[slot];
                wt[u] = WEIGHTED ? wring[slot] : 1.0;
                ring[slot] = load_word(PD + slot);                     // refill PD batches ahead
                if (WEIGHTED) wring[slot] = load_weight(PD + slot);
            }
            // (a counted batch that this loop takes - the last 0-3 of a wavefront's share of them, or every one of them
            // without the split - carries repeat counts: the header's n_one and n_two themselves, whatever lead_mask says)
            if (b + tt * UB < b1) tile_batches<HT, WEIGHTED, HC, DET, UB, ONEWORD>(w, wt, H, PB, lane, s_theta, my_acc, st, zlo, s_ftab, misfit_bits, WEIGHTED ? sets.relax_zero_weight : 0u,
                                                                                   !SPLIT ? 0 : (b + tt * UB < n_one ? 1 : (!ONEWORD && b + tt * UB < n_one + th.n_two() ? 2 : 0)));
        }
        voff += PD * 256;
        asm volatile("" : "+v"(voff));      // keep it one register: the slots stay immediates of the loads
    }
#if defined(GBRS_ABLATE_ATOMICS)
    asm volatile("" ::"v"(st.c[0]), "v"(st.pc[0]));
    st.cidx = st.pidx = 0xFFFFFFFFu;
#endif
    if (DET) {
        if (K < (uint32_t)TILE_WAVES) sc->float_error = 1;      // cannot happen with a deterministic-mode layout
        det_flush<HC>(my_acc, H, lane, st.pidx, st.pc);
        det_flush<HC>(my_acc, H, lane, st.cidx, st.c);
    }
    constexpr int FIRST_FLUSH = 0;
#if defined(GBRS_ABLATE_FLUSH)
    asm volatile("" ::"v"(st.c[0]), "v"(st.pc[0]));
    for (int which = 2; which < 2; ++which) {
#else
    for (int which = FIRST_FLUSH; which < 2 && !DET; ++which) {
#endif
        const uint32_t fidx = which == 0 ? st.pidx : st.cidx;
        if (fidx != 0xFFFFFFFFu) {
            double *ap = my_acc + fidx * H;
#pragma unroll
            for (int h = 0; h < HC; ++h)
                if (h < H) atomicAdd(ap + h, which == 0 ? st.pc[h] : st.c[h]);
        }
    }
    if (st.bad != 0) sc->float_error = 1;
#if defined(GBRS_ESTEP_PRIO)
    __builtin_amdgcn_s_setprio(GBRS_ESTEP_PRIO);
#endif
    __syncthreads();
    GBRS_DIAG_STAMP(2);
    // a locus that lives in this tile only gets its sum stored straight into the A vector the
    // M-step reads; the others go to their slot of `partials` for the fixed-order gather
    uint32_t tix = threadIdx.x;
    asm volatile("" : "+v"(tix));           // opaque: nothing of the epilogue's index arithmetic is hoisted above the batch loop
    for (uint32_t i = tix; i < DH; i += TILE_THREADS) {
        double a = sum_copies<false>(s_acc, i, K, stride);
        // a row without abundance in the tile's leading one-word batches (tile_batches, LEAD): not flagged where it was
        // divided, it left >= 4.49e307 in a sum - as do inf and NaN; a legitimate sum is at most the number of reads.
        // (The one difference from the in-loop flag: a denormal denominator, whose reciprocal was inf before and is
        // 4.49e307 now, is reported.)
        if (SPLIT && estep_theta_regs(UB, HT, DET) && n_lead != 0 && !(a < 4e307)) sc->float_error = 1;
#if defined(GBRS_ABLATE_ATOMICS) || defined(GBRS_ABLATE_BATCHES)
        a = 1.0;                                  // timing-only builds: keep theta finite
#endif
        const uint32_t j = i / H, h = i - j * H;
        const uint32_t d = slot_dest[th.dict_base + j];
        const uint32_t d2 = sets.set_ptr ? sets.dest_b[th.dict_base + j] : 0u;      // (fetched beside d, not after it)
        if constexpr (GATHER) {
            // no slot rows and no gather: a locus that lives in this tile only is stored, every other one added with a
            // global float atomic into its row of this launch's A vector, which the launch before zeroed
            const uint32_t g = ga.gdest[th.dict_base + j];
            const uint32_t g2 = sets.set_ptr ? ga.gdest_b[th.dict_base + j] : 0u;
            auto add = [&](uint32_t gq) {
                double *dst = ga.acc_cur + (size_t)(gq & GSLOT_LOCUS) * H + h;
                if (gq & GSLOT_DIRECT) *dst = a;
                else atomicAdd(dst, a);
            };
            if (sets.set_ptr == nullptr || !(d & (SLOT_SET | SLOT_PAIR))) {
                add(g);
            } else if (d & SLOT_PAIR) {
                add(g);
                add(g2);
            } else {
                const uint32_t *gl = ga.gdest_list + (d & ~SLOT_SET);
                const uint32_t n = gl[0];
                for (uint32_t q = 1; q <= n; ++q) add(gl[q]);
            }
            continue;
        }
        auto put = [&](uint32_t dq) {
            if (dq & SLOT_DIRECT) acc_direct[(size_t)(dq & ~SLOT_DIRECT) * H + h] = a;
            else partials[(size_t)dq * H + h] = a;
        };
        if (sets.set_ptr == nullptr || !(d & (SLOT_SET | SLOT_PAIR))) {
            put(d);
        } else if (d & SLOT_PAIR) {
            // a two-member set: both destinations with the slot (slot_dest and dest_b), no list
            put(d & ~SLOT_PAIR);
            put(d2);
        } else {
            // a larger locus set: its sums go to every member locus, each in a row (or the A element) of its own
            const uint32_t *dl = sets.dest_list + (d & ~SLOT_SET);
            const uint32_t n = dl[0];
            for (uint32_t q = 1; q <= n; ++q) put(dl[q]);
        }
    }
    GBRS_DIAG_STAMP(3);
}

// theta of one dictionary entry at haplotype h, as the tile prologue gathers it: a locus, the sum of a two-member set's
// members (both in the entry: e, e2), or the sum over a larger set's member list (em_layout.h).
template <int HT, bool WEIGHTED>
__device__ __forceinline__ double dict_entry_theta(const double *__restrict__ theta, const SetArgs &sets, uint32_t e, uint32_t e2,
                                                   uint32_t H, uint32_t h) {
    if (sets.set_ptr == nullptr || !(e & (DICT_PAIR | DICT_SET))) return theta[(size_t)e * H + h];
    if (e & DICT_PAIR) {
        const double t0 = theta[(size_t)(e & ~DICT_PAIR) * H + h], t1 = theta[(size_t)e2 * H + h];
        return t0 + t1;
    }
    const uint32_t k = e & ~DICT_SET;
    const uint32_t m0 = sets.set_ptr[k], m1 = sets.set_ptr[k + 1];
    double tv = 0.0;
    constexpr int SETB = (HT == 16 && !WEIGHTED) ? 1 : 4;
    for (uint32_t m = m0; m < m1; m += SETB) {
        uint32_t mem[SETB];
        double tm[SETB];
#pragma unroll
        for (int q = 0; q < SETB; ++q) mem[q] = sets.set_members[min(m + q, m1 - 1)];
#pragma unroll
        for (int q = 0; q < SETB; ++q) tm[q] = theta[(size_t)mem[q] * H + h];
#pragma unroll
        for (int q = 0; q < SETB; ++q) tv += m + q < m1 ? tm[q] : 0.0;
    }
    return tv;
}

// where element i = j * H + h of a tile's theta lives in LDS (planar for 8 / 16 haplotypes, see theta_planar)
template <int HT, bool WEIGHTED>
__device__ __forceinline__ uint32_t theta_lds_index(uint32_t i, uint32_t j, uint32_t h) {
    constexpr uint32_t DP = theta_planar(HT) ? lds_theta_doubles(WEIGHTED, HT) / (HT > 0 ? HT : 1) : 0;
    return theta_planar(HT) ? (((h >> 1) * DP + j) << 1) + (h & 1u) : i;
}

// ---------------------------------------------------------------------------------------------------------------------
// Round 4: the E-step on PERSISTENT workgroups.  tile_estep_kernel gives every tile a workgroup of its own, and a third of
// such a workgroup's life is not the batch loop: kernel arguments + tile header (a scalar load that misses), the sums
// zeroed, dictionary entry -> theta (two dependent round trips), a barrier; at the end the slot destinations (another
// round trip) and the stores - measured exposed, not hidden by the CU's other workgroups (profiles/r03_estep_experiments.txt
// items 10, 15, 17).  Here a launch has as many workgroups as the chip holds at once (n_groups = workgroups per CU x CUs);
// workgroup w walks the tiles w, 2G-1-w, 2G+w, ... of the header array (boustrophedon over the rounds: the headers are
// sorted largest first, so every workgroup gets about the same number of words), and while its wavefronts are in the batch
// loop of one tile the round trips of the NEXT one are in flight:
//   * the next header: a scalar load issued at the top of the tile;
//   * a thread's element of the next dictionary (entry, second member of a pair): vector loads issued at the first ring
//     refill of the loop, and - from them - its theta value(s) at the second refill: they sit in four registers until the
//     loop ends and go to LDS after the barrier that ends the tile (theta of the finished tile is dead by then, so one
//     LDS image suffices);
//   * the thread's slot destination of THIS tile's epilogue: issued before the loop.
// The sums are zeroed where the epilogue reads them (the image is all zero again when the next loop starts), the lanes'
// register state is handed in at the end of every tile exactly as at the end of a tile_estep_kernel workgroup, so the
// arithmetic - and its association - is that kernel's: same tiles, same batches per wavefront, same flush points.
// A tile with more than TILE_THREADS theta elements (or a larger-than-two locus set) gathers the rest in the open, as before.
template <int HT, bool WEIGHTED, bool ONEWORD = false>
__global__ void __launch_bounds__(TILE_THREADS, (HT > 0 && HT <= 8) ? (WEIGHTED ? 4 : GBRS_ESTEP_WAVES) : (WEIGHTED ? 3 : GBRS_ESTEP_WAVES16))
tile_estep_persistent_kernel(uint32_t Hrt, const TileHdr *__restrict__ tiles, const uint32_t *__restrict__ words,
                             const uint32_t *__restrict__ dict, const double *__restrict__ word_weight,
                             const double *__restrict__ theta, double *__restrict__ partials,
                             const uint32_t *__restrict__ slot_dest, int64_t direct_delta /* A vector - partials, in doubles */,
                             EmScalars *__restrict__ sc, uint32_t n_tiles, uint32_t n_groups, ErrArgs ea, SetArgs sets) {
    constexpr int LDS_ACC_DOUBLES = lds_acc_doubles(WEIGHTED, HT);
    constexpr bool PF = HT > 0 && HT <= 8;                  // (the 16-haplotype kernels sit at their register budget)
    constexpr bool EPF = PF && !(HT == 8 && !WEIGHTED && !ONEWORD);   // (... and the multi-word 8-haplotype one has room for the theta registers only)
    __shared__ __attribute__((aligned(16))) double s_theta[lds_theta_doubles(WEIGHTED, HT)];
    __shared__ __attribute__((aligned(16))) double2 s_ftab[32];
    __shared__ __attribute__((aligned(16))) double s_acc[LDS_ACC_DOUBLES];
    __shared__ uint32_t s_stop;
    if (estep_uses_ftab(estep_batches(WEIGHTED, HT), HT) && threadIdx.x < 32) {
        const uint32_t k = threadIdx.x & 15u, sh = (threadIdx.x >> 4) * 2;
        s_ftab[threadIdx.x] = make_double2((double)((k >> sh) & 1u), (double)((k >> (sh + 1)) & 1u));
    }
    if (blockIdx.x >= n_groups) {             // the previous step's deferred error pass rides on this launch
        err_finish_body(ea, blockIdx.x - n_groups);
        return;
    }
    const uint32_t stop_flag = sc->stop;
    const int H = HT > 0 ? HT : (int)Hrt;
    const int PB = pos_bits(H);
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    constexpr int UB = estep_batches(WEIGHTED, HT), PD = WEIGHTED ? GBRS_WEIGHTED_PD : (HT == 16 ? GBRS_H16_PD : GBRS_RAW_PD);
    constexpr int HC = HT > 0 ? HT : 16;
    const uint32_t G = n_groups, me = blockIdx.x;
    uint32_t round = 0, t = me;               // n_groups <= n_tiles: every workgroup has a first tile
    TileHdr th = tiles[t];
    // The word ring of the tile in hand.  It is filled for the FIRST tile here, ahead of everything else, and for every
    // later tile as soon as the previous tile's batch loop ends - before the flush, the barriers and the epilogue - so that a
    // tile's first words are on their way while the workgroup finishes the tile before it (filled only after the closing
    // barrier, every tile start cost each wavefront a bare trip to HBM: ~3 us per tile).
    uint32_t b0, b1;
    __amdgpu_buffer_rsrc_t wres, wtres;
    int voff;
    uint32_t ring[PD];
    double wring[WEIGHTED ? PD : 1];
    auto load_word = [&](int ahead) -> uint32_t {
        return (uint32_t)__builtin_amdgcn_raw_buffer_load_b32(wres, voff + ahead * 256, 0, 0);
    };
    auto load_weight = [&](int ahead) -> double {
        const auto q = __builtin_amdgcn_raw_buffer_load_b64(wtres, 2 * voff + ahead * 512, 0, 0);
        return __hiloint2double((int)q[1], (int)q[0]);
    };
    auto open_tile = [&](const TileHdr &hd) {
        b0 = (uint32_t)(((uint64_t)hd.n_batches * wave) / TILE_WAVES);
        b1 = (uint32_t)(((uint64_t)hd.n_batches * (wave + 1)) / TILE_WAVES);
        const uint32_t *wp = words + (size_t)hd.batch_base * 64;
        const double *wtp = WEIGHTED ? word_weight + (size_t)hd.batch_base * 64 : nullptr;
        wres = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint32_t *>(wp), 0, (int)(b1 * 256u), 0x00020000);
        wtres = __builtin_amdgcn_make_buffer_rsrc(const_cast<double *>(WEIGHTED ? wtp : (const double *)wp), 0,
                                                  WEIGHTED ? (int)(b1 * 512u) : 0, 0x00020000);
        voff = (int)(b0 * 256u) + lane * 4;
#pragma unroll
        for (int u = 0; u < PD; ++u) {
            ring[u] = load_word(u);
            if (WEIGHTED) wring[u] = load_weight(u);
        }
    };
    open_tile(th);
    for (uint32_t i = threadIdx.x; i < (uint32_t)LDS_ACC_DOUBLES; i += TILE_THREADS) s_acc[i] = 0.0;
    {
        // theta of the first tile: nothing to hide it behind
        const uint32_t DH0 = th.template dict_count_of<(PF && !WEIGHTED)>() * H;
        for (uint32_t i = threadIdx.x; i < DH0; i += TILE_THREADS) {
            const uint32_t j = i / H, h = i - j * H;
            const uint32_t e = dict[th.dict_base + j], e2 = sets.set_ptr ? sets.dict_b[th.dict_base + j] : 0u;
            s_theta[theta_lds_index<HT, WEIGHTED>(i, j, h)] = dict_entry_theta<HT, WEIGHTED>(theta, sets, e, e2, H, h);
        }
    }
    if (threadIdx.x == 0) s_stop = stop_flag;
    __syncthreads();
    if (s_stop) return;
    int zlo[32];
#pragma unroll
    for (int k = 0; k < 32; ++k) {
        if constexpr (estep_uses_zlo(estep_batches(WEIGHTED, HT))) asm volatile("v_mov_b32 %0, 0" : "=v"(zlo[k]));
        else zlo[k] = 0;
    }
    const uint32_t misfit_bits = pair_misfit_bits(H, PB, lane);
    LaneAcc<HC> st;
#pragma unroll
    for (int h = 0; h < HC; ++h) st.c[h] = st.pc[h] = 0.0;
    if constexpr (estep_theta_regs(UB, HT, false)) {
#pragma unroll
        for (int h = 0; h < HC / 2; ++h) st.th[h] = theta_pair_t{0.0, 0.0};
    }
    st.cidx = st.pidx = 0xFFFFFFFFu;
    st.bad = 0;
    // a thread's element of a tile's dictionary x haplotype grid is number threadIdx.x: (entry myj, haplotype myh), made
    // where needed (a shift and a mask for the haplotype counts that prefetch)
    // (every use starts from an opaque copy of threadIdx.x: hipcc otherwise hoists the index arithmetic of the epilogue
    // and of the next tile's gather - invariant across the tiles - out of the tile loop and keeps ~20 registers of it
    // alive through the batch loop)
#define GBRS_OPAQUE_TID(name) uint32_t name = threadIdx.x; asm volatile("" : "+v"(name))
    for (;;) {
        const uint32_t rn = round + 1;
        const uint32_t tn = rn * G + ((rn & 1u) ? G - 1u - me : me);
        const bool has_next = tn < n_tiles;                                   // the same for the whole workgroup
        const TileHdr thn = tiles[has_next ? tn : t];                          // scalar load, back long before it is used
        const uint32_t DH = th.template dict_count_of<(PF && !WEIGHTED)>() * H;
        const uint32_t stride = DH | 1u;
        uint32_t K = LDS_ACC_DOUBLES / stride;
        K = K >= 64 ? 64u : (1u << (31 - __clz((int)K)));
        double *my_acc = s_acc + (lane & (K - 1)) * stride;
        // The prefetch registers (clamped indices, not predicates: a branch around a load puts a wait behind it), one step
        // per ring refill:  0: my entry of the next dictionary (+ second member of a pair)  1: theta of it / of both
        // 2: the pair's sum (a larger set: -1.0, summed after the loop), and my slot destination(s) of THIS tile's
        // epilogue into the registers the second member's theta has just left.  At most five registers at a time.
        uint32_t pf_e = 0, pf_e2 = 0, ep_d = 0, ep_d2 = 0;
        double pf_t0 = 0.0, pf_t1 = 0.0;
        int pf_phase = PF ? (has_next ? 0 : 2) : 3;                            // wave-uniform
        auto prefetch_step = [&]() {
            GBRS_OPAQUE_TID(tix);
            const uint32_t myj = tix / (uint32_t)H, myh = tix - myj * (uint32_t)H;
            if (pf_phase == 0) {
                const uint32_t at = thn.dict_base + min(myj, thn.template dict_count_of<(PF && !WEIGHTED)>() - 1u);
                pf_e = dict[at];
                pf_e2 = sets.set_ptr ? sets.dict_b[at] : 0u;
                pf_phase = 1;
            } else if (pf_phase == 1) {
                // a larger set's theta is summed after the loop (rare); its two loads here fetch a valid, unused element
                const bool big = sets.set_ptr != nullptr && (pf_e & DICT_SET) != 0;
                const bool pair = sets.set_ptr != nullptr && (pf_e & DICT_PAIR) != 0;
                const uint32_t l0 = big ? 0u : (sets.set_ptr ? (pf_e & ~(DICT_PAIR | DICT_SET)) : pf_e);
                const uint32_t l1 = pair ? pf_e2 : l0;
                pf_t0 = theta[(size_t)l0 * H + myh];
                pf_t1 = theta[(size_t)l1 * H + myh];
                pf_phase = 2;
            } else {
                if (has_next) {
                    const bool big = sets.set_ptr != nullptr && (pf_e & DICT_SET) != 0;
                    const bool pair = sets.set_ptr != nullptr && (pf_e & DICT_PAIR) != 0;
                    pf_t0 = big ? -1.0 : (pair ? pf_t0 + pf_t1 : pf_t0);        // (theta is never negative)
                }
                if constexpr (EPF) {
                    const uint32_t at = th.dict_base + min(myj, th.template dict_count_of<(PF && !WEIGHTED)>() - 1u);
                    ep_d = slot_dest[at];
                    ep_d2 = sets.set_ptr ? sets.dest_b[at] : 0u;
                }
                pf_phase = 3;
            }
        };
        GBRS_DIAG_PSTAMP(t, 0);
#if defined(GBRS_DIAG_TILE_TIMES)
        if (g_tile_stamps && threadIdx.x == 0) g_tile_stamps[(size_t)t * 8 + 7] = ((unsigned long long)th.template dict_count_of<(PF && !WEIGHTED)>() << 32) | th.n_batches;
#endif
        for (uint32_t b = b0; b < b1; b += PD) {
            if constexpr (PF) {
                if (pf_phase < 3) prefetch_step();
            }
#pragma unroll
            for (int tt = 0; tt < PD / UB; ++tt) {
                uint32_t w[UB];
                double wt[UB];
#pragma unroll
                for (int u = 0; u < UB; ++u) {
                    const int slot = tt * UB + u;
                    w[u] = ring[slot];
                    wt[u] = WEIGHTED ? wring[slot] : 1.0;
                    ring[slot] = load_word(PD + slot);
                    if (WEIGHTED) wring[slot] = load_weight(PD + slot);
                }
                // (one loop here: a batch below the header's n_one, or of the counted two-word run behind it, is read in count
                // form, see the word decode above)
                if (b + tt * UB < b1) tile_batches<HT, WEIGHTED, HC, false, UB, ONEWORD>(w, wt, H, PB, lane, s_theta, my_acc, st, zlo, s_ftab, misfit_bits, WEIGHTED ? sets.relax_zero_weight : 0u,
                                                                                         !(PF && !WEIGHTED) ? 0 : (b + tt * UB < (uint32_t)th.n_one ? 1 : (!ONEWORD && b + tt * UB < (uint32_t)th.n_one + th.n_two() ? 2 : 0)));
            }
            voff += PD * 256;
            asm volatile("" : "+v"(voff));
        }
        if constexpr (PF) {
            while (pf_phase < 3) prefetch_step();                             // a tile with fewer than three refills
        }
        GBRS_DIAG_PSTAMP(t, 1);
        if (has_next) open_tile(thn);                                         // the next tile's first words, under what follows
        // hand in the lanes' sums (the pending set, then the current one), as at the end of a tile_estep_kernel workgroup
        for (int which = 0; which < 2; ++which) {
            const uint32_t fidx = which == 0 ? st.pidx : st.cidx;
            if (fidx != 0xFFFFFFFFu) {
                double *ap = my_acc + fidx * H;
#pragma unroll
                for (int h = 0; h < HC; ++h)
                    if (h < H) atomicAdd(ap + h, which == 0 ? st.pc[h] : st.c[h]);
            }
        }
#pragma unroll
        for (int h = 0; h < HC; ++h) st.c[h] = st.pc[h] = 0.0;
        st.cidx = st.pidx = 0xFFFFFFFFu;
        GBRS_DIAG_PSTAMP(t, 2);
        __syncthreads();
        GBRS_DIAG_PSTAMP(t, 3);
        // ---- epilogue: copies summed in index order and zeroed for the next tile, one store per destination.  A thread's
        // first element and the rest are separate pieces of straight-line code: where the prefetched and the fetched-now
        // forms meet in one loop body, hipcc waits for EVERYTHING in flight (s_waitcnt vmcnt(0): the next tile's words just
        // requested, the stores just issued - ~1 us each time).
        auto deliver = [&](uint32_t i, double a, uint32_t d, uint32_t d2) __attribute__((always_inline)) {
            const uint32_t j = i / H, h = i - j * H;
            auto put = [&](uint32_t dq) __attribute__((always_inline)) {
                // (one store at partials + [direct_delta]: written as two stores, or as a choice between the two array pointers,
                // hipcc 7.2 parks the pointers in scratch and picks one with an indexed load)
                const int64_t at = (int64_t)((size_t)(dq & ~SLOT_DIRECT) * H + h) + ((dq & SLOT_DIRECT) ? direct_delta : (int64_t)0);
                partials[at] = a;
            };
            if (sets.set_ptr == nullptr || !(d & (SLOT_SET | SLOT_PAIR))) {
                put(d);
            } else if (d & SLOT_PAIR) {
                put(d & ~SLOT_PAIR);
                put(d2);
            } else {
                const uint32_t *dl = sets.dest_list + (d & ~SLOT_SET);
                const uint32_t n = dl[0];
                for (uint32_t q = 1; q <= n; ++q) put(dl[q]);
            }
        };
        GBRS_OPAQUE_TID(tix_e);
        if constexpr (EPF) {
            if (tix_e < DH) deliver(tix_e, sum_copies<true>(s_acc, tix_e, K, stride), ep_d, ep_d2);
        }
        for (uint32_t i = tix_e + (EPF ? TILE_THREADS : 0); i < DH; i += TILE_THREADS) {
            const uint32_t j = i / H;
            const uint32_t d = slot_dest[th.dict_base + j];
            const uint32_t d2 = sets.set_ptr ? sets.dest_b[th.dict_base + j] : 0u;      // (fetched beside d, not after it)
            deliver(i, sum_copies<true>(s_acc, i, K, stride), d, d2);
        }
        GBRS_DIAG_PSTAMP(t, 4);
        if (!has_next) break;
        // ---- theta of the next tile into LDS: my element from the registers, the rest (tiles with more than TILE_THREADS
        // elements, larger sets) gathered now
        const uint32_t DHn = thn.template dict_count_of<(PF && !WEIGHTED)>() * H;
        GBRS_OPAQUE_TID(tix_n);
        bool from_regs = false;
        if constexpr (PF) {
            from_regs = !(pf_t0 < 0.0);
            if (tix_n < DHn && from_regs) {
                const uint32_t j = tix_n / H, h = tix_n - j * H;
                s_theta[theta_lds_index<HT, WEIGHTED>(tix_n, j, h)] = pf_t0;
            }
        }
        for (uint32_t i = tix_n + (from_regs ? TILE_THREADS : 0); i < DHn; i += TILE_THREADS) {
            const uint32_t j = i / H, h = i - j * H;
            const uint32_t e = dict[thn.dict_base + j], e2 = sets.set_ptr ? sets.dict_b[thn.dict_base + j] : 0u;
            s_theta[theta_lds_index<HT, WEIGHTED>(i, j, h)] = dict_entry_theta<HT, WEIGHTED>(theta, sets, e, e2, H, h);
        }
        GBRS_DIAG_PSTAMP(t, 5);
        __syncthreads();
        GBRS_DIAG_PSTAMP(t, 6);
        th = thn;
        t = tn;
        round = rn;
    }
    if (st.bad != 0) sc->float_error = 1;
#undef GBRS_OPAQUE_TID
}

// Rows with more than MAX_ROW_WORDS loci: one wavefront per row, global float64 atomics into
// acc_extra (rare: a read aligning to > 32 isoforms).
template <bool ONES>
__global__ void __launch_bounds__(256)
long_rows_estep_kernel(uint64_t n_long, uint32_t H, const uint64_t *__restrict__ long_ptr,
                       const uint32_t *__restrict__ long_loc, const uint32_t *__restrict__ long_mask,
                       const double *__restrict__ long_weight, const double *__restrict__ theta,
                       double *__restrict__ acc_extra, EmScalars *__restrict__ sc, uint32_t relax_zero_weight) {
    if (!ONES && sc->stop) return;
    const uint64_t row = (uint64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (row >= n_long) return;
    const int lane = threadIdx.x & 63;
    const uint64_t p0 = long_ptr[row], p1 = long_ptr[row + 1];
    double s = 0.0;
    for (uint64_t p = p0 + lane; p < p1; p += 64) {
        const uint32_t m = long_mask[p];
        const double *tp = theta + (size_t)long_loc[p] * H;
        for (uint32_t h = 0; h < H; ++h)
            if ((m >> h) & 1u) s += ONES ? 1.0 : tp[h];
    }
    const double den = wave_sum_all(s);
    if (!(den > 0.0)) {
        // (resampling handles: a zero-weight row takes no part, its own zero denominator is no float error)
        if (lane == 0 && !(relax_zero_weight && long_weight[row] == 0.0)) sc->float_error = 1;
        return;
    }
    const double v = long_weight[row] / den;
    for (uint64_t p = p0 + lane; p < p1; p += 64) {
        const uint32_t m = long_mask[p];
        double *ap = acc_extra + (size_t)long_loc[p] * H;
        for (uint32_t h = 0; h < H; ++h)
            if ((m >> h) & 1u) atomicAdd(ap + h, v);
    }
}

// Deterministic mode: the long rows one after another on a single wavefront.  A row's loci are
// distinct, so the lanes of one step never meet, and the steps of one wave reach an address in program
// order: the sums are added in row order on every launch.
template <bool ONES>
__global__ void __launch_bounds__(64)
long_rows_estep_serial_kernel(uint64_t n_long, uint32_t H, const uint64_t *__restrict__ long_ptr,
                              const uint32_t *__restrict__ long_loc, const uint32_t *__restrict__ long_mask,
                              const double *__restrict__ long_weight, const double *__restrict__ theta,
                              double *__restrict__ acc_extra, EmScalars *__restrict__ sc, uint32_t relax_zero_weight) {
    if (!ONES && sc->stop) return;
    const int lane = threadIdx.x & 63;
    for (uint64_t row = 0; row < n_long; ++row) {
        const uint64_t p0 = long_ptr[row], p1 = long_ptr[row + 1];
        double s = 0.0;
        for (uint64_t p = p0 + lane; p < p1; p += 64) {
            const uint32_t m = long_mask[p];
            const double *tp = theta + (size_t)long_loc[p] * H;
            for (uint32_t h = 0; h < H; ++h)
                if ((m >> h) & 1u) s += ONES ? 1.0 : tp[h];
        }
        const double den = wave_sum_all(s);
        if (!(den > 0.0)) {
            if (lane == 0 && !(relax_zero_weight && long_weight[row] == 0.0)) sc->float_error = 1;
            continue;
        }
        const double v = long_weight[row] / den;
        for (uint64_t p = p0 + lane; p < p1; p += 64) {
            const uint32_t m = long_mask[p];
            double *ap = acc_extra + (size_t)long_loc[p] * H;
            for (uint32_t h = 0; h < H; ++h)
                if ((m >> h) & 1u) atomicAdd(ap + h, v);
        }
    }
}

// acc[l][h] for the loci the tile epilogues did not finish themselves (locus_class: 0 no slot,
// 1 one slot = already in acc, 2 few slots, 3 many slots), + acc_extra from the long-row kernel.
// Blocks [0, light_blocks): one thread per (l, h) element, either of every locus (classes 0-2; when
// the whole vector is about to be all-reduced) or of the class-2 loci only (compact list); the
// remaining blocks: one wavefront per class-3 locus, slots spread over 64/HP
// lanes and reduced in fixed order.
__global__ void __launch_bounds__(256)
gather_kernel(uint32_t L, uint32_t H, uint32_t HP, uint32_t light_blocks, uint32_t heavy_blocks, uint32_t n_heavy,
              int all_elements, uint32_t n_light, const uint32_t *__restrict__ light_loci,
              const uint32_t *__restrict__ slot_ptr,
              const uint32_t *__restrict__ heavy_loci, const uint8_t *__restrict__ locus_class,
              const double *__restrict__ partials, const double *__restrict__ acc_extra,
              double *__restrict__ acc, const EmScalars *__restrict__ sc, int honour_stop) {
    if (honour_stop && sc->stop) return;
    if (blockIdx.x < light_blocks) {
        uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
        uint32_t l, h;
        if (all_elements) {
            if (i >= (uint64_t)L * H) return;
            l = (uint32_t)(i / H);
            h = (uint32_t)(i - (uint64_t)l * H);
        } else {                                    // only the loci with 2..HEAVY_SLOTS slots
            if (i >= (uint64_t)n_light * H) return;
            const uint32_t li = (uint32_t)(i / H);
            h = (uint32_t)(i - (uint64_t)li * H);
            l = light_loci[li];
            i = (uint64_t)l * H + h;
        }
        const uint32_t cls = locus_class[l];
        if (cls == 3) return;
        double a = acc_extra ? acc_extra[i] : 0.0;
        if (cls == 1) {
            a += acc[i];
        } else if (cls == 2) {
            const uint32_t k0 = slot_ptr[l], k1 = slot_ptr[l + 1];
            for (uint32_t k = k0; k < k1; ++k) a += partials[(size_t)k * H + h];
        }
        acc[i] = a;
        return;
    }
    const uint32_t hv = (blockIdx.x - light_blocks) * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (hv >= n_heavy) return;
    const uint32_t l = heavy_loci[hv];
    const int lane = threadIdx.x & 63;
    const uint32_t h = lane & (HP - 1), sub = lane / HP, nsub = 64 / HP;
    const uint32_t k0 = slot_ptr[l], k1 = slot_ptr[l + 1];
    double a = 0.0;
    if (h < H) {
        // four independent chains per lane over the locus's consecutive slot rows
        double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
        uint32_t k = k0 + sub;
        for (; k + 3 * nsub < k1; k += 4 * nsub) {
            const uint32_t s0 = k, s1 = k + nsub, s2 = k + 2 * nsub, s3 = k + 3 * nsub;   // consecutive rows
            a0 += partials[(size_t)s0 * H + h];
            a1 += partials[(size_t)s1 * H + h];
            a2 += partials[(size_t)s2 * H + h];
            a3 += partials[(size_t)s3 * H + h];
        }
        for (; k < k1; k += nsub) a0 += partials[(size_t)k * H + h];
        a = (a0 + a1) + (a2 + a3);
    }
    for (uint32_t off = HP; off < 64; off <<= 1) a += __shfl_xor(a, off, WAVE);
    if (sub == 0 && h < H) {
        const size_t i = (size_t)l * H + h;
        acc[i] = a + (acc_extra ? acc_extra[i] : 0.0);
    }
}
