// The HMM handle (private to the library): the core state of hmm.hip - tables, emissions, the last run's arrays - and one
// part per pass of hmm_passes.hip, with the descriptors those buffers hold and the little the passes share with the core.
#pragma once
#include "common.h"
#include "hmm_route.h"

namespace gbrs {

constexpr double TINY = 4.9406564584124654e-324;   // np.nextafter(0, 1)
constexpr int MAX_H = 16;   // S <= 136 (CC-style 16 founders); DO is H = 8, S = 36
typedef double mfma_d4 __attribute__((ext_vector_type(4)));   // accumulator of v_mfma_f64_16x16x4_f64 (MFMA sweeps, hmm_match.inc)

struct ChromDesc {
    int64_t gene_off;     // offset of the chromosome's first gene in the per-sample gene axis
    int64_t trans_off;    // offset (in S*S blocks) of tprob[c][0] in the transition buffer
    int64_t bp_off;       // offset (in S entries) of the chromosome's backpointer rows
    int64_t chunk_off;    // offset (in BT_B-row chunks) of the chromosome's backtrace chunk maps
    int32_t n_genes, n_trans;
    // Blocked scan (hmm_blocked.inc): a descriptor may stand for a run of genes of a chromosome whose recursion starts
    // from an injected boundary vector instead of the chromosome's own start / end.
    int32_t inject;       // -1: the natural start; else the slot of the block's boundary vector
    int32_t real_chrom;   // the chromosome whose last gene this descriptor ends on (forward / delta), else -1
};

struct BlockRange {                // blocked scan (hmm_blocked.inc)
    int64_t gene_off, trans_off;   // of the chromosome
    int32_t lo, hi, n;             // genes [lo, hi) of a chromosome of n genes
    int32_t chrom;
    int32_t direct;                // 1: chained directly from the chromosome's own start (forward structure: its first block) /
                                   // end (backward structure: its last block) while the other blocks' operators are built:
                                   // it has no operator, and the combine takes its boundary vector from what the chain stored
    int64_t bp_off;                // of the chromosome's backpointer rows
};

struct GridChrom {               // grid pass (hmm_grid.inc): one per chromosome of the handle
    int64_t gene_off;            // its first gene row within a sample's gamma
    int32_t knot_off, n_knots;   // its knots in the handle's knot arrays; n_knots = 0: the chromosome is not on the grid
    int32_t point_off, n_points; // its grid points among the grid points of the handle's chromosomes, handle order
};

struct GridTile {                // a run of at most P consecutive grid points of one chromosome: one wavefront's work
    int32_t chrom, first;
};

struct MatchChrom {              // match pass (hmm_match.inc): one per chromosome ON the grid: a chromosome without grid points gets no tile
    int64_t k_off, k_len;        // its columns within a row
    int32_t chrom;               // its index on the handle
};

struct SnpChrom {                // SNP imputation (hmm_impute.inc): one per chromosome of the handle
    int64_t gene_off;            // its first gene row within a sample's gamma
    int32_t knot_off, n_knots;   // its knots in the handle's SNP knot arrays; n_knots = 0: the chromosome has no SNP
    int64_t snp_off;             // its first SNP among the handle's SNPs (handle order)
};

}  // namespace gbrs

struct gbrs_hmm {
    int device = 0;
    hipStream_t stream = nullptr, stream_b = nullptr, stream_c = nullptr;   // see hmm_launch
    hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    hipEvent_t ev_fork = nullptr, ev_b = nullptr, ev_c1 = nullptr, ev_c = nullptr;
    hipEvent_t ev_ops[2] = {nullptr, nullptr};   // blocked scan: the alpha / backward operator kernels are done
    int H = 0, S = 0, n_chrom = 0, n_samples = 0;
    std::vector<gbrs::ChromDesc> chroms;
    int64_t total_genes = 0, total_trans = 0, total_bp = 0, total_chunks = 0;
    int max_bp_rows = 0;                      // max over chromosomes of min(n_genes, n_trans)
    bool have_eprob = false, ran = false;
    bool pe_ready = false;                    // peprob = exp(eprob) is current (the emission kernels write both)
    bool logs_ready = false;                  // alpha / beta / scaler of the last run have been made (hmm_make_logs)
    gbrs::DevBuf<gbrs::ChromDesc> d_chroms;
    gbrs::DevBuf<int32_t> d_order;            // chromosome indices, longest first
    gbrs::DevBuf<double> tprob, pprob, pprob_t, init_vec;   // log T, exp(T), exp(T) transposed per block
    gbrs::DevBuf<double> tprob_q;             // S = 36 / 136: log T in the chain kernels' lane order (pprob, pprob_t too)
    bool quad = false;                        // tables are in lane order
    gbrs::DevBuf<double> amat_f, amat_b;      // S = 36, large batches: the MFMA operands of exp(T) and its transpose (made on first use)
    gbrs::DevBuf<double> expr, avecs, eprob, peprob, xsum, bhat, alpha, beta, gamma, delta, scaler, invz;
    double *expr_stage = nullptr;      // pinned host image of `expr` for small batches (gbrs_hmm_set_expression)
    size_t expr_stage_n = 0;
    gbrs::DevBuf<double> bscale, bcorr;       // free-running backward: per-gene scale and log correction
    gbrs::DevBuf<uint8_t> has_avec;
    gbrs::DevBuf<uint16_t> bp, bt_exit;       // backpointers; per-chunk exit maps of the backtrace
    gbrs::DevBuf<int32_t> last_state, states, calls;
    double t_emis = 0, t_fwd = 0, t_bwd = 0, t_bt = 0, t_run = 0;
    // blocked scan (hmm_blocked.inc; 36 states, up to HMM_BLOCKED_MAX samples): the chromosomes cut into blocks
    // Two block structures (round 4): the forward one (alpha, delta) may open every chromosome with a long block that is
    // chained DIRECTLY from the chromosome's start while the other blocks' operators are being built (no operator for it);
    // the backward one closes every chromosome with such a block.  [0] forward, [1] backward.
    int n_vb = 0, blk_samples = 0;            // n_vb: the larger of the two block counts (buffers are sized by it)
    int n_blk[2] = {0, 0}, n_head[2] = {0, 0};
    // The last run's route.  What later calls read from it: free_backward() - beta needs bcorr; Blocked - the backward chains
    // started from injected vectors; BlockedRank - gbrs_hmm_info reports how the fix-ups went; tie_check - dspec_tie holds
    // the flags of the backtrace's margin check; delta_interleaved - how `delta` is laid out.
    gbrs::HmmRoute last;
    gbrs::DevBuf<gbrs::BlockRange> d_ranges[2];
    gbrs::DevBuf<int32_t> d_first_block[2];   // blocks of chromosome c: first_block[c] .. first_block[c+1]
    gbrs::DevBuf<int32_t> d_vorder[2];        // block indices, the directly chained ones first (n_head of them)
    gbrs::DevBuf<gbrs::ChromDesc> d_vfwd, d_vbwd;   // the blocks as descriptors of the forward / delta and of the backward chains
    std::vector<gbrs::BlockRange> h_ranges0;  // host copy of d_ranges[0]
    gbrs::DevBuf<double> dspec_c;             // rank-convergence delta: every block's constant against the block before it,
    gbrs::DevBuf<int32_t> dspec_g, dspec_fail;   // the gene from which its stored values stand, per (sample, chromosome) failure flags
    gbrs::DevBuf<int32_t> dspec_tie;          // per (sample, chromosome): a decision of the path inside the error of the blocks' vectors
    hipStream_t stream_h[3] = {nullptr, nullptr, nullptr};   // the direct chains of alpha / backward / delta
    hipEvent_t ev_head[3] = {nullptr, nullptr, nullptr};
    // Pipelined batch pass (round 4, hmm_launch_groups): the chromosomes in two groups of consecutive chromosomes, each with
    // its own emission -> chains -> posterior / backtrace pipeline on its own three streams, so that the emission of the
    // second group and the posteriors / backtraces of whichever group is done run beside the chains that set the pass's length.
    bool emission_pending = false;            // gbrs_hmm_set_expression left the emission kernel to the next run
    double em_thr = 0.0, em_sigma = 0.0;
    int n_groups = 0;
    int grp_lo[2] = {0, 0}, grp_hi[2] = {0, 0}, grp_order_off[2] = {0, 0}, grp_max_bp[2] = {0, 0};
    gbrs::DevBuf<int32_t> d_order_grp;        // per group: its chromosomes, longest first
    hipStream_t stream_g[3] = {nullptr, nullptr, nullptr};   // the second group's streams (the first uses stream / stream_b / stream_c)
    hipEvent_t gev_em[2] = {nullptr, nullptr}, gev_b[2] = {nullptr, nullptr}, gev_c[2] = {nullptr, nullptr},
               gev_done[2] = {nullptr, nullptr}, gev_start = nullptr;
    gbrs::DevBuf<double> g_f, g_b, g_d, inj_f, inj_b, inj_d;   // block operators [sample][block][36][36], boundary vectors [sample][block][36]
    gbrs::DevBuf<int32_t> e_f, e_b;           // power-of-two exponents of the operators' columns

    // ---- the passes over the last run (hmm_passes.hip); `ms` is the device time of a part's last call --------------------
    // Grid pass (hmm_grid.inc): the marker grid is sample independent and stays here like avecs; the two output buffers
    // are sized by the last call that asked for them.
    struct Grid {
        bool have = false;
        int tiles = 0;
        int64_t points = 0;                   // grid points of the handle's chromosomes
        gbrs::DevBuf<gbrs::GridChrom> d_chroms;
        gbrs::DevBuf<gbrs::GridTile> d_tiles;
        gbrs::DevBuf<double> knot_x, x, dosage, gamma;
        gbrs::DevBuf<int32_t> knot_gene;
        double ms = 0;
        bool dosage_ready = false;            // dosage holds the last run's dosages for `dosage_sample` (-1: all)
        int dosage_sample = -1;
        void invalidate() { dosage_ready = false; }
    } grid;
    // Match pass (hmm_match.inc): the panel's dosages in grid.dosage's row layout, its norms, the outputs of the last call
    struct Match {
        int n_panel = 0;
        bool vec2 = false;                    // rows and chromosome starts are 16-byte aligned (even H)
        gbrs::DevBuf<double> panel, cross, snorm;
        gbrs::DevBuf<gbrs::MatchChrom> d_chroms;
        std::vector<double> panel_norm;       // [n_panel][n_chrom]
        double ms = 0;
    } match;
    // SNP imputation (hmm_impute.inc): positions, patterns and the knot above every SNP stay here like the grid (16 B per
    // SNP), with the knots and their gene rows; d is D[n][total_genes][H], the founder dosages at the genes of the
    // last run, made by the first gbrs_hmm_impute call after a run and kept for its later chunks; out holds one chunk
    struct Snp {
        int64_t n = 0;
        gbrs::DevBuf<gbrs::SnpChrom> d_chroms;
        gbrs::DevBuf<double> knot_x, x, d, out;
        gbrs::DevBuf<int32_t> knot_row, idx;
        gbrs::DevBuf<uint32_t> mask;
        bool d_ready = false;                 // d holds the last run's dosages for `d_sample` (-1: all)
        int d_sample = -1;
        double ms_setup = 0, ms_d = 0, ms_kernel = 0;   // the last set_snps; D and the kernel of the last pass
        void invalidate() { d_ready = false; }
    } snp;
    // The founder-change table of the path draws and of the pair pass, made by whichever asks first (ensure_change_table)
    gbrs::DevBuf<uint8_t> change_tab;
    // Path draws (hmm_sample.inc): the buffers hold one slab of draws
    struct Draws {
        gbrs::DevBuf<uint8_t> cols, paths;
        gbrs::DevBuf<int32_t> changes;
        gbrs::DevBuf<uint32_t> streams;
        gbrs::DevBuf<unsigned long long> degenerate;
        double ms = 0;
    } draws;
    // Diagnostics (hmm_diag.inc): the device images of the five outputs, [n][total_genes] each, and the pair posteriors
    // of one (sample, chromosome); sized by the last call that asked for them
    struct Diag {
        gbrs::DevBuf<double> xo, pswitch, errlod, maxprob, xi;
        gbrs::DevBuf<int32_t> maxmarg;
        double ms = 0;
    } diag;
    // Log-likelihood (hmm_loglik.inc): the sums of the last call, and the candidate tables of one chromosome as uploaded
    // (t) and as exp() transposed per block (pt); they grow to the largest call and are reused
    struct Loglik {
        gbrs::DevBuf<double> out, t, pt;
        double ms = 0;
    } ll;
};

namespace gbrs {

// What the handle keeps of a run stops being that run's, in two steps.  New emissions (gbrs_hmm_set_expression,
// gbrs_hmm_set_eprob) and a call of gbrs_hmm_run drop what the passes cached from the posteriors: a part that caches
// something per run adds its invalidate() here.
inline void hmm_invalidate_dosages(gbrs_hmm *h) {
    h->grid.invalidate();
    h->snp.invalidate();
}
// A run's launch begins, everything it needs is prepared: the log-domain arrays go too.  Not sooner: a run that fails
// while it prepares leaves the last run's arrays, `ran` and logs standing, and hmm_make_logs is not made to run twice
// on one run (the blocked route rescales bscale in place).
inline void hmm_invalidate_run(gbrs_hmm *h) {
    h->logs_ready = false;
    hmm_invalidate_dosages(h);
}

// alpha, beta and the scaler of the last run, made on the first call after it (hmm.hip)
int hmm_make_logs(gbrs_hmm *h);

}  // namespace gbrs
