// Which kernels a pass of the `gbrs reconstruct` HMM runs (hmm.hip): the tuning switches, read from the
// environment once per entry point, and the route a pure function resolves from them and the handle's
// shape.  Host only - no HIP include, so a plain C++ compiler builds it (tests/native/hmm_route_driver.cpp).
#pragma once

#include <algorithm>
#include <climits>
#include <cstdlib>
#include <cstring>

namespace gbrs {

// ---- compile-time defaults of the switches (a -D on the command line overrides: scripts/) ----------------------

#ifndef HMM_BATCH_MIN
#define HMM_BATCH_MIN 24  // below this every sample gets waves of its own (measured: 16 samples 3.4 vs 3.6 ms, 32 samples 5.1 vs 4.8 ms)
#endif
#ifndef HMM_MFMA_MIN
#define HMM_MFMA_MIN 64   // 36 states, at least this many samples: alpha and backward sweeps of 16 samples per wave on MFMA (see the kernels' comment)
#endif
#ifndef HMM_DLANES_MIN
#define HMM_DLANES_MIN 64 // 36 states, at least this many samples: delta chain with the samples on the lanes (measured with the MFMA sweeps beside it:
                          // 8-32 samples the one-state-per-lane kernels win, 64 a wash, 128: 10.3 vs 12.1 ms, 256: 19.4 vs 22.1 ms)
#endif
#ifndef HMM_BPL_MIN
#define HMM_BPL_MIN 32        // samples from which viterbi_bp_lanes_kernel replaces viterbi_bp_kernel
#endif
#ifndef HMM_MFMA_NG2_MIN
#define HMM_MFMA_NG2_MIN (1 << 30)   // samples from which a wavefront of the MFMA sweeps carries two groups of 16: never by
#endif                               // default - measured (round 4): 256 samples 16.3-16.7 ms either way, 128: 9.2 -> 12.0, 64: 6.9 -> 9.3

#ifndef HMM_BLOCKED_MAX
#define HMM_BLOCKED_MAX 4     // 36 states, at most this many samples: the blocked scan (the sum-product operators cost 36 columns per block and sample;
                              // round 4, Viterbi values by rank convergence: 0.63 / 1.01 / 1.51 / 1.85 ms at 1 / 2 / 3 / 4 samples against 1.9-2.0 on the
                              // chains; 5 samples 2.25 against 2.0)
#endif
#ifndef HMM_DELTA_AFTER_OPS
#define HMM_DELTA_AFTER_OPS 0     // measured: 0.653 against 0.630 ms (the operators do not get faster without the delta chains beside them)
#endif
#ifndef HMM_DELTA_INTERLEAVED
#define HMM_DELTA_INTERLEAVED 0     // delta as [gene][sample] for the large batches: parity-green, no gain (15.72 against 15.73 ms), off
#endif
#ifndef HMM_BP_AFTER_SWEEPS
#define HMM_BP_AFTER_SWEEPS 0
#endif
#ifndef HMM_XCD_SPAN
#define HMM_XCD_SPAN 2        // XCDs a chromosome's sample groups are spread over under GBRS_TUNING_HMM_XCD (1, 2 or 4)
#endif
#ifndef HMM_XCD_GRIDS
#define HMM_XCD_GRIDS 0       // batch chain kernels on XCD-aware 1-D grids (GBRS_TUNING_HMM_XCD)
#endif
#ifndef HMM_DELTA_SPEC
#define HMM_DELTA_SPEC 1      // blocked scan: Viterbi values by rank convergence (one chain per block + fix-up) instead of max-plus block operators
#endif
#ifndef HMM_BLOCK_GENES
#define HMM_BLOCK_GENES 40    // genes per block aimed at (at most HMM_BLOCKS_MAX blocks per chromosome)
#endif
#ifndef HMM_BLOCKS_MAX
#define HMM_BLOCKS_MAX 64
#endif
#ifndef HMM_HEAD_PERCENT
#define HMM_HEAD_PERCENT 0    // share of a chromosome's genes that is chained directly while the operators of the rest are built.
                              // Round 4: built (GBRS_TUNING_HMM_HEAD=20..60), parity-green, SLOWER - beside the operator kernels,
                              // which keep every CU and the memory system busy, a directly chained block runs at ~1.7 us per step
                              // instead of 0.4 (wave priority, s_setprio 3, did not change that): 40k genes, one sample 1.06 ms without,
                              // 1.19 / 1.42 / 1.64 / 1.85 ms with 20 / 30 / 40 / 50 % (profiles/r04_hmm_experiments.txt)
#endif
#ifndef HMM_PIPE_MIN
// Samples from which a batch pass runs as two pipelined chromosome groups (emission of group 2 beside the sweeps of group 1).
// Parity-green and measured slower on one MI355X (256 samples 19.75-19.88 against 16.43-16.53 ms, 128: 13.14-13.18 against
// 9.21-9.31; profiles/r04_hmm_experiments.txt item 4), so never by default: GBRS_TUNING_HMM_PIPELINE=<samples> switches it on.
#define HMM_PIPE_MIN (1 << 30)
#endif
#ifndef HMM_PIPE_FIRST_PERCENT
#define HMM_PIPE_FIRST_PERCENT 30   // share of the genes in the group that goes first (the one with the longest chromosome)
#endif

// ---- tuning: every GBRS_TUNING_HMM_* / GBRS_DIAG_HMM_* value ---------------------------------------------------

struct HmmTuning {
    // smallest batch that takes ... (INT_MAX: never)
    int mfma_min = HMM_MFMA_MIN;            // MFMA: the MFMA sweeps - the parity tests run them at 16
    int dlanes_min = HMM_DLANES_MIN;        // DLANES: the samples-on-lanes delta chain
    int bplanes_min = HMM_BPL_MIN;          // BPLANES: the samples-on-lanes backpointer kernel
    int pipe_min = HMM_PIPE_MIN;            // PIPELINE: the emission left to the run, two pipelined chromosome groups
    int blocked_max = HMM_BLOCKED_MAX;      // BLOCKED: largest batch that takes the blocked scan (0: never)
    int mfma_ng = 0;                        // MFMA_NG = 1 / 2 forces the sample groups of 16 per wavefront; 0: HMM_MFMA_NG2_MIN decides
    // DELTA_SPEC=0: the blocked scan's delta through max-plus block operators (round 3) instead of rank convergence
    bool delta_spec = HMM_DELTA_SPEC != 0;
    // DELTA_TOL=<absolute tolerance> of the fix-up's convergence test (negative: no block ever converges - every chromosome
    // takes the fallback chain; the tests use it)
    double delta_tol_abs = 1e-9, delta_tol_rel = 1e-13;
    // DELTA_AFTER_OPS=1: the delta side (the short one) behind the two operator kernels instead of beside them - measured:
    // the operators are no faster alone (backward side 0.556 against 0.563 ms) and the forward side gets longer (0.549
    // against 0.496): off.
    bool delta_after_ops = HMM_DELTA_AFTER_OPS != 0;
    // BP_AFTER=1: the backpointer kernel (one sample per lane: a cache line and a page per lane and load) behind the sweeps
    // instead of beside them
    bool bp_after = HMM_BP_AFTER_SWEEPS != 0;
    bool back_after = false;                // BACK_AFTER=1: the backward sweep behind the alpha sweep
    bool serial = false;                    // SERIAL=1: the three chains on one stream
    // DELTA_ROWS=1: delta as [gene][sample] where both its writer and its reader are the samples-on-lanes kernels (measured: no gain)
    bool delta_interleaved = HMM_DELTA_INTERLEAVED != 0;
    int xcd_mask = HMM_XCD_GRIDS;           // XCD: the batch chain kernels on XCD-aware 1-D grids; 1: sweeps, 2: delta chain
    int xcd_span = HMM_XCD_SPAN;            // XCD_SPAN: 1, 2 or 4
    int block_genes = HMM_BLOCK_GENES, blocks_max = HMM_BLOCKS_MAX, head_pct = HMM_HEAD_PERCENT;   // BLOCK_GENES, BLOCKS_MAX, HEAD
    int pipe_first_pct = HMM_PIPE_FIRST_PERCENT;                                                   // PIPE_FIRST
#if defined(GBRS_DIAG_BUILD)                 // never in the product library: the switches give wrong results (timing only)
    // GBRS_DIAG_HMM_INTERLEAVED=1: the batch kernels address the per-sample arrays as [gene][sample], a step's 16 rows
    // contiguous - the other kernels keep [sample][gene]
    bool diag_interleaved = false;
    // GBRS_DIAG_HMM_SKIP=<letters of a, b, c, p, v>: leave the alpha / backward / delta chain, the posterior, the
    // backpointers + backtrace out of the pass
    char diag_skip[8] = "";
    bool skips(char c) const { return std::strchr(diag_skip, c) != nullptr; }
#else
    bool skips(char) const { return false; }
#endif
};

namespace hmm_env {
// "threshold, set but <= 0 means never"
inline void threshold(const char *name, int &v) {
    if (const char *e = std::getenv(name); e) v = std::atoi(e) > 0 ? std::atoi(e) : INT_MAX;
}
// a flag with a compile-time default
inline void flag(const char *name, bool &v) {
    if (const char *e = std::getenv(name); e) v = std::atoi(e) != 0;
}
// an integer taken only from [lo, hi]
inline void in_range(const char *name, int lo, int hi, int &v) {
    if (const char *e = std::getenv(name); e && std::atoi(e) >= lo && std::atoi(e) <= hi) v = std::atoi(e);
}
}  // namespace hmm_env

// Read at every entry point (gbrs_hmm_set_expression, gbrs_hmm_run) and never kept: the tests change the variables
// between runs of one process.
inline HmmTuning hmm_tuning_from_env() {
    using namespace hmm_env;
    HmmTuning t;
    threshold("GBRS_TUNING_HMM_MFMA", t.mfma_min);
    threshold("GBRS_TUNING_HMM_DLANES", t.dlanes_min);
    threshold("GBRS_TUNING_HMM_BPLANES", t.bplanes_min);
    threshold("GBRS_TUNING_HMM_PIPELINE", t.pipe_min);
    if (const char *e = std::getenv("GBRS_TUNING_HMM_BLOCKED"); e) t.blocked_max = std::atoi(e);
    in_range("GBRS_TUNING_HMM_MFMA_NG", 1, 2, t.mfma_ng);
    flag("GBRS_TUNING_HMM_DELTA_SPEC", t.delta_spec);
    if (const char *e = std::getenv("GBRS_TUNING_HMM_DELTA_TOL"); e) {
        t.delta_tol_abs = std::atof(e);
        if (t.delta_tol_abs < 0.0) t.delta_tol_rel = 0.0;
    }
    flag("GBRS_TUNING_HMM_DELTA_AFTER_OPS", t.delta_after_ops);
    flag("GBRS_TUNING_HMM_BP_AFTER", t.bp_after);
    flag("GBRS_TUNING_HMM_BACK_AFTER", t.back_after);
    flag("GBRS_TUNING_HMM_SERIAL", t.serial);
    flag("GBRS_TUNING_HMM_DELTA_ROWS", t.delta_interleaved);
    if (const char *e = std::getenv("GBRS_TUNING_HMM_XCD"); e) t.xcd_mask = std::atoi(e);
    if (const char *e = std::getenv("GBRS_TUNING_HMM_XCD_SPAN"); e && (std::atoi(e) == 1 || std::atoi(e) == 2 || std::atoi(e) == 4))
        t.xcd_span = std::atoi(e);
    in_range("GBRS_TUNING_HMM_BLOCK_GENES", 2, INT_MAX, t.block_genes);
    in_range("GBRS_TUNING_HMM_BLOCKS_MAX", 1, INT_MAX, t.blocks_max);
    if (const char *e = std::getenv("GBRS_TUNING_HMM_HEAD"); e) t.head_pct = std::max(0, std::min(90, std::atoi(e)));
    in_range("GBRS_TUNING_HMM_PIPE_FIRST", 1, 99, t.pipe_first_pct);
#if defined(GBRS_DIAG_BUILD)
    flag("GBRS_DIAG_HMM_INTERLEAVED", t.diag_interleaved);
    if (const char *e = std::getenv("GBRS_DIAG_HMM_SKIP"); e)
        for (const char *c = "abcpv"; *c; ++c)
            if (std::strchr(e, *c)) t.diag_skip[std::strlen(t.diag_skip)] = *c;
#endif
    return t;
}

// ---- route ------------------------------------------------------------------------------------------------------

struct HmmShape {
    int S, H, n_samples, n_chrom;
    long long total_trans;
};

// who runs the alpha and the backward sweep
enum class HmmSweep {
    Generic,   // any state count: forward_viterbi_kernel (delta and the backpointers in the same sweep) + backward_kernel, one stream
    Quad,      // 136 states: the quad chains
    Wave,      // 36 / 28 / 10 / 6 states: the single-wave chains, one sample or HMM_SB samples per wave (HmmRoute::batched)
    Blocked,   // 36 states, few samples: the blocked scan (hmm_blocked.inc)
    Mfma,      // 36 states, many samples: 16 samples (HmmRoute::mfma_groups times) per wave on MFMA
};
// who runs the delta chain
enum class HmmDelta {
    WithSweep,     // the Generic / Quad family's own
    Wave,          // the single-wave chain, one sample or HMM_SB samples per wave as the sweeps
    Lanes,         // the samples on the lanes
    BlockedRank,   // blocked scan: one chain per block + fix-up (rank convergence)
    BlockedOps,    // blocked scan: max-plus block operators
};
// who writes the backpointers
enum class HmmBp {
    WithSweep,   // forward_viterbi_kernel
    Chains,      // the blocked scan's delta chains, in the same pass over T
    Quad, Wave, Lanes, Generic,   // viterbi_bp_quad_kernel / _wave_kernel / _lanes_kernel / viterbi_bp_kernel behind the delta chain
};

struct HmmRoute {
    HmmSweep sweep = HmmSweep::Generic;
    HmmDelta delta = HmmDelta::WithSweep;
    HmmBp bp = HmmBp::WithSweep;
    // Few samples: one sample per wave (latency).  Many samples: HMM_SB samples share each wave's
    // transition registers (half the block loads per sample; measured best of 1-8 at 64 samples).
    bool batched = false;
    int mfma_groups = 0;              // Mfma: sample groups of 16 per wavefront, 1 or 2
    // the emission gbrs_hmm_set_expression left to the run is made per chromosome group: two pipelined groups
    // (hmm_launch_groups), which are made of the MFMA sweeps and the samples-on-lanes kernels
    bool grouped = false;
    // delta as [gene][sample] (a step's / a gene's rows contiguous: the backpointer kernel reads one page per gene instead of
    // one per lane); gbrs_hmm_get copies a sample's rows out with a stride.  Otherwise [sample][gene].
    bool delta_interleaved = false;
    bool chain_interleaved = false;   // diagnostic builds only (GBRS_DIAG_HMM_INTERLEAVED)
    int xcd_mask = 0, xcd_span = 1;
    // Blocked: the backtrace checks the margins of the path it writes against these tolerances (TieCheck)
    bool tie_check = false;
    double tol_abs = 0.0, tol_rel = 0.0;
    bool serial = false, back_after = false, bp_after = false, delta_after_ops = false;   // stream ordering

    bool free_backward() const { return sweep != HmmSweep::Generic; }   // those sweeps rescale on their own (beta_corr_kernel)
};

// gbrs_hmm_set_expression: a large 36-state batch leaves its emission kernel to the run.  `batch_emission`: the batch
// takes emission_batch_kernel (the kernel the grouped pass launches).
inline bool hmm_defers_emission(const HmmShape &s, const HmmTuning &t, bool batch_emission) {
    return batch_emission && s.S == 36 && s.n_samples >= t.pipe_min && s.n_chrom >= 2 && s.total_trans > 0;
}

// gbrs_hmm_run.  `emission_deferred`: what hmm_defers_emission said when the expression was set; a deferred emission is
// made up in one launch (hmm_flush_emission) when the route is not the grouped one.
inline HmmRoute hmm_route(const HmmShape &s, const HmmTuning &t, bool emission_deferred) {
    HmmRoute r;
    r.serial = t.serial;
    r.back_after = t.back_after;
    r.bp_after = t.bp_after;
    const int ns = s.n_samples;
    const bool wave = s.S == 36 || s.S == 28 || s.S == 10 || s.S == 6;
    if (s.S == 136) {
        r.sweep = HmmSweep::Quad;
        r.bp = HmmBp::Quad;
    }
    if (!wave) return r;
    // the MFMA sweeps, the samples-on-lanes kernels and the blocked scan are written for 36 states; the lanes chain
    // and the MFMA sweeps go before the blocked scan, which excludes both
    const bool s36 = s.S == 36 && s.total_trans > 0;
    const bool mfma = s36 && ns >= t.mfma_min;
    const bool dlanes = s36 && ns >= t.dlanes_min;
    const bool blocked = s36 && !mfma && !dlanes && ns <= t.blocked_max;
    r.batched = ns >= HMM_BATCH_MIN;
    r.sweep = mfma ? HmmSweep::Mfma : blocked ? HmmSweep::Blocked : HmmSweep::Wave;
    r.grouped = emission_deferred && mfma && dlanes && t.mfma_ng != 2;
    if (mfma) r.mfma_groups = r.grouped ? 1 : t.mfma_ng ? t.mfma_ng : ns >= HMM_MFMA_NG2_MIN ? 2 : 1;
    r.delta = dlanes ? HmmDelta::Lanes : !blocked ? HmmDelta::Wave : t.delta_spec ? HmmDelta::BlockedRank : HmmDelta::BlockedOps;
    const bool bplanes = s36 && ns >= t.bplanes_min;
    r.bp = blocked ? HmmBp::Chains : bplanes ? HmmBp::Lanes : HmmBp::Generic;
    if (!blocked && !r.grouped && ns <= 4) r.bp = HmmBp::Wave;
    r.delta_interleaved = t.delta_interleaved && !r.grouped && r.delta == HmmDelta::Lanes && r.bp == HmmBp::Lanes;
    r.xcd_mask = t.xcd_mask;
    r.xcd_span = t.xcd_span;
    // The blocked scan's vectors are the sequential chain's up to rounding (and, by rank convergence, up to the fix-up's
    // acceptance spread), so a decision of the backtrace that the sequential chain takes by less than that - an exact
    // tie, which its first-index rule decides, or a near-tie - may fall the other way: see hmm_launch.
    r.tie_check = blocked && !t.skips('v');
    r.tol_abs = t.delta_tol_abs;
    r.tol_rel = t.delta_tol_rel;
    r.delta_after_ops = t.delta_after_ops;
#if defined(GBRS_DIAG_BUILD)
    r.chain_interleaved = t.diag_interleaved && !r.grouped;
    r.delta_interleaved = r.delta_interleaved || r.chain_interleaved;
#endif
    return r;
}

}  // namespace gbrs
