// What gbrs_em_create* decides before any device work (em.hip) and the rules the tile layout's build applies to the
// numbers it reads back from the device (em_layout.hip): the GBRS_TUNING_* variables of the EM handle, read from the
// environment once per create, and the plan a pure function resolves from them and the handle's shape.  This is the one
// place that reads those variables; the handle keeps the plan, and what each of its steps launches is resolved from it in
// em_step.h.  Host only - no HIP include, so a plain C++ compiler builds it
// (tests/native/em_plan_driver.cpp).
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstdlib>

#include "../../include/gbrs_hip.h"

namespace gbrs {

// ---- tuning: every GBRS_TUNING_* value that create and the layout build read ------------------------------------------

struct EmTuning {
    struct Int {   // a variable and whether it was set at all
        bool set = false;
        int v = 0;
        bool is(int x) const { return set && v == x; }
        bool nonzero() const { return set && v != 0; }
    };
    int dict_cap = 0;           // DICT_CAP: at most this many loci per tile dictionary (taken when above a row's words)
    Int locus_sets;             // LOCUS_SETS=1: the whole-row form of the locus sets, taken; 0: that form is not taken
    Int group_sets;             // GROUP_SETS=1 / 0: the mask-group sets taken whatever they save / not looked for
    uint32_t set_min_rows = 192;   // SET_MIN_ROWS (> 0): rows a mask-group set must be carried by
    Int run_words;              // RUN_WORDS=0 no fold, 1 the one-word fold alone, 2 both folds - forced
    int tile_words = 0;         // TILE_WORDS (>= 64): words per tile instead of the rule's
    bool tile_cut = true;       // TILE_CUT=0: the two-grid cut even where the rule chooses the tile size
    int tile_target = 0;        // TILE_TARGET (>= 1): the cut aims at this many tiles instead of the chip's places
    bool tile_order = true;     // TILE_ORDER=0 keeps the tiles in locus order
    bool half_loci = false;     // HALF_LOCI=1: 16 haplotypes as half-loci of 8
    bool persistent = false;    // PERSISTENT=1: persistent E-step workgroups
    unsigned persistent_groups = 0;   // PERSISTENT_GROUPS (> 0): that many of them
    bool no_phase_split = false;      // NO_PHASE_SPLIT=1: one batch loop for every batch
    uint32_t resample_cut = 256;      // RESAMPLE_CUT (> 0): rows with a larger count get a workgroup in the draw
    bool no_fused_mstep = false;      // NO_FUSED_MSTEP=1: gather and M-step as separate launches (em_step.h)
    bool no_float_check = false;      // NO_FLOAT_CHECK set at all: no "row without abundance" error (ablation builds of the E-step)
    bool no_gather_mstep = false;     // NO_GATHER_MSTEP=1: the M-step stays a launch of its own (em_step.h, em_gather_mstep)
    // STRIPES=S (2, 4 or 8): that stripe on every counted run whatever the size or the cap; 0: no stripes; "S1,S2": the
    // one-word runs and the pair runs apart (the measurements of profiles/estep_stripes.txt).  -1: the rule (em_take_stripes)
    int stripes_one = -1, stripes_two = -1;
};

namespace em_env {
inline EmTuning::Int integer(const char *name) {
    EmTuning::Int i;
    if (const char *e = std::getenv(name); e) { i.set = true; i.v = std::atoi(e); }
    return i;
}
// a value taken only when it is at least `lo`
template <typename T>
inline void at_least(const char *name, int lo, T &v) {
    if (const char *e = std::getenv(name); e && std::atoi(e) >= lo) v = (T)std::atoi(e);
}
// a stripe: 0, 2, 4 or 8; anything else leaves the rule in charge
inline int stripe_value(const char *e) {
    const int v = std::atoi(e);
    return (v == 0 && *e == '0') || v == 2 || v == 4 || v == 8 ? v : -1;
}
}  // namespace em_env

// Read at every gbrs_em_create* and never kept: the tests change the variables between handles of one process.
inline EmTuning em_tuning_from_env() {
    using namespace em_env;
    EmTuning t;
    at_least("GBRS_TUNING_DICT_CAP", 1, t.dict_cap);
    t.locus_sets = integer("GBRS_TUNING_LOCUS_SETS");
    t.group_sets = integer("GBRS_TUNING_GROUP_SETS");
    at_least("GBRS_TUNING_SET_MIN_ROWS", 1, t.set_min_rows);
    t.run_words = integer("GBRS_TUNING_RUN_WORDS");
    at_least("GBRS_TUNING_TILE_WORDS", 64, t.tile_words);
    t.tile_cut = !integer("GBRS_TUNING_TILE_CUT").is(0);
    at_least("GBRS_TUNING_TILE_TARGET", 1, t.tile_target);
    t.tile_order = !integer("GBRS_TUNING_TILE_ORDER").is(0);
    t.half_loci = integer("GBRS_TUNING_HALF_LOCI").nonzero();
    t.persistent = integer("GBRS_TUNING_PERSISTENT").nonzero();
    at_least("GBRS_TUNING_PERSISTENT_GROUPS", 1, t.persistent_groups);
    t.no_phase_split = integer("GBRS_TUNING_NO_PHASE_SPLIT").nonzero();
    at_least("GBRS_TUNING_RESAMPLE_CUT", 1, t.resample_cut);
    t.no_fused_mstep = integer("GBRS_TUNING_NO_FUSED_MSTEP").nonzero();
    t.no_float_check = integer("GBRS_TUNING_NO_FLOAT_CHECK").set;
    t.no_gather_mstep = integer("GBRS_TUNING_NO_GATHER_MSTEP").nonzero();
    if (const char *e = std::getenv("GBRS_TUNING_STRIPES"); e) {
        t.stripes_one = t.stripes_two = stripe_value(e);
        for (const char *c = e; *c; ++c)
            if (*c == ',') { t.stripes_two = stripe_value(c + 1); break; }
    }
    return t;
}

// ---- shape ----------------------------------------------------------------------------------------------------------------

// the dictionary limits of em_layout.h for one (weighted, haplotypes) pair: those functions are __host__ __device__, so
// the caller evaluates them
struct EmDictLimits {
    uint32_t max_row_words = 0;   // max_row_words(H)
    uint32_t index_limit = 0;     // dict_index_limit(H)
    uint32_t lds_doubles = 0;     // lds_theta_doubles(weighted, H)
    uint32_t det_cap = 0;         // det_dict_cap(H, weighted)
};

struct EmShape {
    uint32_t H = 0, L = 0;
    uint64_t R = 0, N = 0;        // N: the entries after the upload (masked handles: the masked count)
    uint32_t flags = 0;           // GBRS_EM_*
    bool counts_given = false;    // the caller passed row counts
    int n_cu = 0;                 // compute units of the handle's device
    uint32_t tile_words = 0, tile_words_max = 0, tile_rounds_min = 1;   // TILE_WORDS, TILE_WORDS_MAX, TILE_ROUNDS_MIN
    uint32_t err_blocks = 0;      // error-pass workgroups that ride a step's tile launch (em.hip, ERR_BLOCKS)
    EmDictLimits dict;            // at H haplotypes, weighted as em_weighted() says
    EmDictLimits dict_half;       // at H / 2 haplotypes, unweighted: the half-locus view's (read at H = 16 only)
};

// per-row weights: counts given, a resampling handle (base weights of counts or ones) or identical rows merged
inline bool em_weighted(uint32_t flags, bool counts_given) {
    return counts_given || (flags & (GBRS_EM_RESAMPLE | GBRS_EM_MERGE_IDENTICAL_ROWS)) != 0;
}

// ---- plan -----------------------------------------------------------------------------------------------------------------

struct EmPlan {
    bool tiled = false;              // the tile layout; false: the CSC kernels (nothing below is used)
    // 16 haplotypes as half-loci on the 8-haplotype kernels (em_layout.h; the review's "two halves of 8"): built, parity-green,
    // NO gain - one GPU's shard of config 5: E-step 0.1518 ms against 0.1525 (the words double, the cost per word halves) and
    // the iteration 0.1997 against 0.1744 (gather and M-step as two launches over every element).  GBRS_TUNING_HALF_LOCI=1
    // switches it on; weighted rows and the deterministic mode never take it.
    uint32_t view = 1;               // 2: the layout is built over tL = 2 L half-loci of tH = H / 2 haplotypes
    uint32_t tH = 0, tL = 0;
    // Row order inside a tile: the stream order (gbrs_hip.h) by default - every lane walks a contiguous piece of the
    // tile's sorted rows, so it stays on one locus list for long stretches (E-step on C2: raw reads 0.158 -> 0.152 ms,
    // merged distinct rows 0.110 -> 0.056 ms against the interleaved order that used to be their default).
    int row_order = 2;               // 0 sorted, 1 interleaved, 2 streams
    bool merge = false, deterministic = false, weighted = false;
    unsigned side_by_side = 1;       // handles that share the device (GBRS_EM_SIDE_BY_SIDE: 2)
    // locus sets (weighted rows never: their tiles are dictionary-bound)
    bool locus_sets = false;
    bool whole_row_sets = false;     // step 3b's first form instead of step 3c's mask groups
    bool group_sets = false;         // step 3c is looked at
    bool group_sets_forced = false;
    int sets_forced = -1;            // whole-row form: 1 / 0 the choice is forced, -1 the rule decides
    uint32_t set_min_rows = 192;
    // folds of identical one- and two-word reads
    bool counted_pairs = false;      // the layout's kernels read TileHdr::n_two
    bool fold = false;               // the fold is tried ...
    int fold_mode = 3;               // ... first as merge_flag_kernel's mode 3 (both folds) or 2 (one-word reads)
    bool fold_forced = false;        // what is tried is taken
    // resident E-step workgroups per CU (tile_estep_kernel's launch bounds: 3 for unweighted rows of <= 8 haplotypes,
    // else 2) and the places the chip has for them in TILE_ROUNDS_MIN rounds
    unsigned per_cu = 3;
    uint64_t places = 0;
    uint32_t tile_words = 0, tile_words_cap = 0;   // the tile-size rule's bounds (cap: a multiple of 64 follows from the rule)
    uint32_t tile_words_forced = 0;  // > 0: GBRS_TUNING_TILE_WORDS, clamped
    // The cut (em_layout.hip, stage 7).  exact_cut: tiles end at tile_words words or at d_max DISTINCT dictionary ids,
    // whichever comes first, and the size is rescaled until about tile_target tiles come out - one round of the chip's
    // places beside the error-pass workgroups.  false (GBRS_TUNING_TILE_WORDS forces the size, or GBRS_TUNING_TILE_CUT=0):
    // the two-grid cut - a tile starts where the word offset passes a multiple of the tile size or the per-list entry
    // count a multiple of dseg.
    bool exact_cut = false;
    uint64_t tile_target = 0;
    bool tile_target_forced = false; // GBRS_TUNING_TILE_TARGET: the exact cut whatever the sample's size (em_take_exact_cut)
    bool reorder_tiles = true;       // launch order: most batches first
    uint32_t d_max = 0, dseg = 0;    // dictionary capacity; what is left of it beside one row's loci
    bool dict_room = false;          // false: d_max leaves no room for a row's loci - the build refuses
    // persistent E-step workgroups: one per place the chip has for them, shared between handles that run side by side.
    // GBRS_TUNING_PERSISTENT=1 switches them on: built, parity-green and measured in round 4 - 8-10 % SLOWER than one
    // workgroup per tile on the C2 sample (profiles/r04_estep_experiments.txt), so off by default
    uint32_t persist_groups = 0;
    // GBRS_TUNING_NO_PHASE_SPLIT=1: the E-step takes every tile's n_one and n_two as 0 - one batch loop, as before the headers
    // had the field (A/B in one build, and the cross-check of the two-loop form in the tests)
    uint32_t lead_mask = ~0u;
    uint32_t resample_cut = 256;     // (the variable is read by a resampling handle with counts only)
    bool no_fused_mstep = false, no_float_check = false;   // EmTuning's, for the handle's steps (em_step.h, em_check_float)
    bool no_gather_mstep = false;
    // Stripes (em_layout.hip, tile_pad_kernel; em_take_stripes below): in a tile's counted runs a group of rows - one
    // dictionary id, or one (first id, second id) pair - starts only at a cell that is a multiple of S, so that the lanes
    // of a wavefront change id in the same batches.  -1: S per tile and run by em_stripe_pick; 0: none; 2, 4, 8: forced.
    // Both 0 in every layout without counted_pairs.
    int stripes_one = 0, stripes_two = 0;
    bool stripes_forced = false;     // GBRS_TUNING_STRIPES asked for a stripe: taken whatever the sample's size
};

// Tiles the exact cut aims at: one round of the places a handle has - its share when handles run side by side - less the
// error-pass workgroups that ride the same launch (a chip with no more places than those keeps them all).
// GBRS_TUNING_TILE_TARGET overrides.
inline uint64_t em_tile_target(uint64_t places, unsigned side_by_side, uint32_t err_blocks, int forced) {
    if (forced > 0) return (uint64_t)forced;
    const uint64_t n = std::max<uint64_t>(places / std::max(side_by_side, 1u), 1);
    return n > err_blocks ? n - err_blocks : n;
}

inline EmPlan em_plan(const EmShape &s, const EmTuning &t) {
    EmPlan p;
    const uint32_t f = s.flags;
    p.merge = (f & GBRS_EM_MERGE_IDENTICAL_ROWS) != 0;
    p.deterministic = (f & GBRS_EM_DETERMINISTIC) != 0;
    p.weighted = em_weighted(f, s.counts_given);
    p.side_by_side = (f & GBRS_EM_SIDE_BY_SIDE) ? 2u : 1u;
    p.no_fused_mstep = t.no_fused_mstep;
    p.no_float_check = t.no_float_check;
    p.no_gather_mstep = t.no_gather_mstep;
    if ((f & GBRS_EM_RESAMPLE) && s.counts_given) p.resample_cut = t.resample_cut;
    p.tiled = !(f & GBRS_EM_LAYOUT_CSC) && s.H <= 16 && s.N < 0xFFFFFFFFull;
    p.tH = s.H;
    p.tL = s.L;
    if (!p.tiled) return p;

    if (f & GBRS_EM_FORCE_INTERLEAVE) p.row_order = 1;
    else if (f & GBRS_EM_NO_STREAMS) p.row_order = (p.weighted && !(f & GBRS_EM_NO_INTERLEAVE)) ? 1 : 0;
    if (s.H == 16 && t.half_loci && !p.weighted && !p.deterministic && (uint64_t)s.L * 2 < (1u << 27)) p.view = 2;
    p.tH = s.H / p.view;
    p.tL = s.L * p.view;
    const EmDictLimits &d = p.view == 2 ? s.dict_half : s.dict;

    p.locus_sets = !(f & GBRS_EM_NO_LOCUS_SETS) && !p.weighted;
    p.whole_row_sets = p.locus_sets && t.locus_sets.is(1);
    if (t.locus_sets.set) p.sets_forced = t.locus_sets.v != 0;
    p.group_sets = p.locus_sets && !t.group_sets.is(0);      // (and only when step 3b took no sets)
    p.group_sets_forced = t.group_sets.is(1);
    p.set_min_rows = t.set_min_rows;

    p.counted_pairs = p.row_order == 2 && !p.weighted && !p.deterministic && p.view == 1 &&
                      (p.tH == 1 || p.tH == 2 || p.tH == 4 || p.tH == 8);
    p.fold = !(f & GBRS_EM_NO_RUN_WORDS) && p.counted_pairs && !t.run_words.is(0);
    p.fold_mode = t.run_words.is(1) ? 2 : 3;
    p.fold_forced = t.run_words.set;
    if (p.counted_pairs) {
        p.stripes_one = t.stripes_one;
        p.stripes_two = t.stripes_two;
        p.stripes_forced = t.stripes_one > 0 || t.stripes_two > 0;
    }

    p.per_cu = (p.weighted || p.tH > 8) ? 2u : 3u;
    const unsigned n_cu = (unsigned)std::max(s.n_cu, 1);
    p.places = (uint64_t)s.tile_rounds_min * p.per_cu * n_cu;
    p.tile_words = s.tile_words;
    // (weighted rows - merged reads, EC counts - stay at 16,320: the merged C2 sample reads 0.0345 ms there, 0.0357 at 20,900)
    p.tile_words_cap = p.weighted ? std::min<uint32_t>(s.tile_words_max, 16320) : s.tile_words_max;
    if (t.tile_words) p.tile_words_forced = std::min<uint32_t>((uint32_t)t.tile_words, s.tile_words_max);
    p.exact_cut = t.tile_cut && !p.tile_words_forced;
    p.tile_target = em_tile_target(p.places, p.side_by_side, s.err_blocks, t.tile_target);
    p.tile_target_forced = t.tile_target > 0;
    p.reorder_tiles = t.tile_order;

    p.d_max = std::min<uint32_t>(1024, d.lds_doubles / p.tH);
    p.d_max = std::min(p.d_max, d.index_limit);     // what a word's index field can hold (1024 at H = 16)
    if (p.deterministic) p.d_max = std::min(p.d_max, d.det_cap);
    if (t.dict_cap > (int)d.max_row_words) p.d_max = std::min(p.d_max, (uint32_t)t.dict_cap);
    p.dict_room = p.d_max > d.max_row_words;
    p.dseg = p.dict_room ? p.d_max - d.max_row_words : 0;

    unsigned groups = p.per_cu * n_cu / p.side_by_side;
    if (t.persistent_groups) groups = t.persistent_groups;
    p.persist_groups = t.persistent ? std::max(groups, 1u) : 0u;
    p.lead_mask = t.no_phase_split ? 0u : ~0u;
    return p;
}

// ---- the rules that need a number from the device -----------------------------------------------------------------------

// Tile size: as large as still leaves TILE_ROUNDS_MIN rounds of the chip's resident E-step workgroups, between TILE_WORDS
// and the cap (em_layout.h), a multiple of 64; GBRS_TUNING_TILE_WORDS overrides.  Handles that run side by side - the
// locus ranges of one sample - fill the rounds together.
inline uint32_t em_tile_words(const EmPlan &p, uint64_t total_words) {
    if (p.tile_words_forced) return p.tile_words_forced;
    const uint64_t fit = total_words * p.side_by_side / p.places;
    return (uint32_t)std::min<uint64_t>(std::max<uint64_t>(fit, p.tile_words), p.tile_words_cap) & ~63u;
}

// The exact cut's sizes.  A pass cuts candidates on the word grid and splits those whose distinct ids pass d_max, so it can
// end with more tiles than it aimed at; the next pass enlarges the size in proportion.  At most TILE_CUT_PASSES passes.
constexpr int TILE_CUT_PASSES = 3;
// The exact cut is for the samples whose words fit ONE round under the cap.  A sample of several rounds keeps the two-grid
// cut: its tiles, about half as long, fill the last round better than tiles of the full cap do.  Measured
// (profiles/estep_tile_cut.txt, five alternations, iterations/s, two-grid against exact cut): multi-isoform reads, 59.6 M
// words, 3,497 against 1,835 tiles: 6,594-6,627 against 6,121-6,133; 25 M reads x 16 haplotypes, 28.5 M words, 2,261
// against 1,009 tiles: 6,618-6,645 against 5,913-5,947.  In one round: the bench sample 25,372-25,529 against
// 26,282-26,622, merged rows 24,402-24,594 against 25,226-25,469, deterministic 1,196-1,198 against 1,372-1,375.
// GBRS_TUNING_TILE_TARGET takes the exact cut whatever the size.
inline bool em_take_exact_cut(const EmPlan &p, uint64_t total_words) {
    if (!p.exact_cut) return false;
    return p.tile_target_forced || (total_words + p.tile_target - 1) / p.tile_target <= p.tile_words_cap;
}
inline uint32_t em_cut_clamp(const EmPlan &p, uint64_t words) {
    return (uint32_t)std::min<uint64_t>(std::max<uint64_t>((words + 63) & ~63ull, p.tile_words), p.tile_words_cap);
}
// first pass: the smallest multiple of 64 that fits total_words into tile_target tiles, in [TILE_WORDS, cap]
inline uint32_t em_cut_tile_words(const EmPlan &p, uint64_t total_words) {
    return em_cut_clamp(p, (total_words + p.tile_target - 1) / p.tile_target);
}
// after a pass at tile_words that gave `tiles`: the size of the next pass, or tile_words itself when the pass met the
// target or no larger size is left
inline uint32_t em_cut_rescale(const EmPlan &p, uint32_t tile_words, uint64_t tiles) {
    if (tiles <= p.tile_target) return tile_words;
    return std::max(tile_words, em_cut_clamp(p, ((uint64_t)tile_words * tiles + p.tile_target - 1) / p.tile_target));
}

// The fold pays by the words it takes away - one for a one-word read, two for a two-word read - and a launch still wants
// a tile of TILE_WORDS words for every resident workgroup place of the chip: a sample smaller than that is launch-bound
// and keeps one word per read.  GBRS_TUNING_RUN_WORDS=2 / 1 forces the choice (0 never gets here).
inline bool em_take_fold(const EmPlan &p, uint64_t words_in, uint64_t folded) {
    if (p.fold_forced) return true;
    return folded * 100 >= words_in * 15 && (words_in - folded) * p.side_by_side / p.places >= (uint64_t)p.tile_words;
}

// Stripes (EmPlan::stripes_one).  They pad, so they are for the samples the batch loop dominates: the layouts whose kernels
// read the counted runs, and - em_take_fold's own size clause - not the launch-bound ones, which keep their layout cell for
// cell.  words: the layout's words after the folds.  GBRS_TUNING_STRIPES=2 / 4 / 8 forces them, 0 switches them off.
inline bool em_take_stripes(const EmPlan &p, uint64_t words) {
    if (!p.counted_pairs || (p.stripes_one == 0 && p.stripes_two == 0)) return false;
    if (p.stripes_forced) return true;
    return words * p.side_by_side / p.places >= (uint64_t)p.tile_words;
}
// Which S a run of `words` rows takes in one tile: the largest of 4 and 2 whose padded cells (cells4, cells2: every
// group rounded up to the stripe) stay within (1 + STRIPE_CAP) x the run's rows - a sample whose ids carry a word or two
// each would double otherwise.  forced: 0, 2, 4, 8 as the plan says, -1 the rule.  (constexpr: the build's kernel calls it.)
// Measured on the bench sample (profiles/estep_stripes.txt; iterations/s, three runs each, taken in turn; S of the one-word
// runs, S of the pair runs): (0, 0) 30,696-30,765; (4, 0) 32,776-33,233; (0, 4) 33,394-33,477; (2, 2) 33,964-34,118;
// (8, 2) 34,243-34,357; (4, 2) 34,610-34,810; (4, 4) 35,105-35,133 at 1.059 and 1.146 cells per word.  A cap of 1/8 gave
// the pair runs S = 4 in some tiles and 2 in most; 1/4 gives every run of that sample S = 4.
constexpr uint32_t STRIPE_CAP_NUM = 1, STRIPE_CAP_DEN = 4;
constexpr bool em_stripe_fits(uint64_t cells, uint64_t words) {
    return cells * STRIPE_CAP_DEN <= words * (STRIPE_CAP_DEN + STRIPE_CAP_NUM);
}
constexpr uint32_t em_stripe_pick(int forced, uint64_t words, uint64_t cells4, uint64_t cells2) {
    if (forced >= 0) return (uint32_t)forced;
    return em_stripe_fits(cells4, words) ? 4u : em_stripe_fits(cells2, words) ? 2u : 0u;
}

// Whole-row sets (step 3b).  A set entry costs its tile a longer prologue and epilogue (its members' theta summed, its
// sums stored once per member), which pays when the words it saves are many and every dictionary entry serves many
// words.  Measured (profiles/r03_estep_experiments.txt item 8): C2, 23 % fewer words at 137 words per id: E-step -11 %;
// the 16-haplotype shard (same saving, 62 words per id) +8 %; multi-isoform reads (9 % fewer words) +8 %.  And no more
// sets than twice the loci: many thin sets fill the tiles' dictionaries (item 16 of the same file).
// P / P2: the pairs before and after, V: the sets, L: the loci.  GBRS_TUNING_LOCUS_SETS=1 / 0 forces the choice.
inline bool em_use_whole_row_sets(const EmPlan &p, uint64_t P, uint64_t P2, uint64_t L, uint64_t V) {
    if (p.sets_forced >= 0) return p.sets_forced != 0;
    return P2 * 100 <= P * 85 && P2 >= 100 * (L + V) && V <= 2 * L;
}

// Mask-group sets (step 3c): the frequent sets only, and no more of them than half the loci - the rows a set must be
// carried by double until they fit (GBRS_TUNING_GROUP_SETS=1: whatever the first threshold keeps)
inline bool em_group_sets_fit(const EmPlan &p, uint64_t V, uint64_t L) { return V * 2 <= L || p.group_sets_forced; }
// ... and worth it when they take a twentieth of the words away
inline bool em_use_group_sets(const EmPlan &p, uint64_t P, uint64_t P2) { return p.group_sets_forced || P2 * 100 <= P * 95; }

}  // namespace gbrs
