/*
 * gbrs_hip.h - C ABI of libgbrs_hip.so: the MI355X (gfx950) implementation of the two
 * numeric hot paths of churchill-lab/gbrs.
 *
 * The reference has no FFI seam (it is pure Python); the entry points below are cut at the
 * seams its own callers use, so a maintainer can bind them with ctypes and
 * keep `gbrs quantify` / `gbrs reconstruct` unchanged above this line.  All citations are
 * relative to /root/reference/src/gbrs/.
 *
 *   EM  (gbrs quantify -M 4):   emase/EMfactory.py:20-287 as driven from
 *                                gbrs/emase_utils.py:282-316
 *   HMM (gbrs reconstruct):     gbrs/gbrs_utils.py:463-599
 *
 * Conventions
 *   - plain pointers and sizes only; the caller owns every host buffer, the library copies in
 *     during the call and never keeps a host pointer after it returns;
 *   - every function returns 0 on success and a negative gbrs_status on failure, with the text
 *     available from gbrs_last_error() (thread-local).  The Python shim turns that into the
 *     RuntimeError / FloatingPointError the reference would have raised;
 *   - calls are blocking and synchronous unless the name ends in _async; one HIP stream per
 *     handle; different handles may be driven from different threads (ctypes drops the GIL);
 *   - matrices named "H x L" are row-major with the haplotype index slowest, exactly the
 *     ndarray layout of EMfactory.allelic_expression.
 */
#ifndef GBRS_HIP_H
#define GBRS_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GBRS_ABI_VERSION 5

enum gbrs_status {
    GBRS_OK = 0,
    GBRS_ERR_INVALID = -1,      /* bad argument (RuntimeError in the reference)            */
    GBRS_ERR_HIP = -2,          /* HIP runtime failure, message carries hipGetErrorString  */
    GBRS_ERR_NO_DEVICE = -3,    /* no gfx950 device visible: there is NO CPU fallback      */
    GBRS_ERR_FLOAT = -4,        /* 0/0 or overflow where the reference's np.seterr(all='raise')
                                   (EMfactory.py:256) raises FloatingPointError              */
    GBRS_ERR_UNSUPPORTED = -5,  /* not available on this handle or in this mode: models 1-3
                                   without gbrs_em_set_groups, or with GBRS_EM_DETERMINISTIC */
    GBRS_ERR_STATE = -6         /* call order violated (e.g. run before prepare)           */
};

const char *gbrs_last_error(void);
int gbrs_abi_version(void);
/* Number of visible HIP devices, or a negative status. */
int gbrs_device_count(void);
/* Optional: pays the process's one-time device costs now (runtime start-up, context, loading the library's code
 * objects, the first small copy) - about 0.1-0.3 s that otherwise land in the first create call.  The Python host
 * calls it on a thread while the input files are read. */
int gbrs_warm_up(int device);

/* ------------------------------------------------------------------------------------------
 * EM: EMASE Model 4 over the alignment incidence tensor.
 * ---------------------------------------------------------------------------------------- */

typedef struct gbrs_em gbrs_em_t;

/* flags for gbrs_em_create* */
#define GBRS_EM_DEFAULT 0u
/* Merge rows with identical alignment patterns into one weighted row while building the device
 * layout (what `gbrs compress`, gbrs/emase_utils.py:60-103, does as a separate command).  Same
 * fixed point; off by default: the default layout keeps its rows unweighted and counts every read
 * in every iteration (identical one-word reads may share one word that carries their number, see
 * GBRS_EM_NO_RUN_WORDS). */
#define GBRS_EM_MERGE_IDENTICAL_ROWS 1u
/* Keep the reference's CSC arrays as the device layout (two passes with global float64 atomics).
 * The default is the packed-row-tile layout; this one is the simple cross-check. */
#define GBRS_EM_LAYOUT_CSC 2u
/* Tuning switches for the order of rows inside a tile.
 * Stream order (default): rows are grouped by length and each group of 64/len lanes walks its own
 * contiguous run of the tile's sorted rows over successive batches, so a lane stays on one locus
 * list for long stretches and the per-lane register accumulation rarely spills to LDS atomics.
 * GBRS_EM_NO_STREAMS falls back to the previous defaults: sorted order for raw reads, interleaved
 * order (locus lists dealt round-robin across the 64 lanes of a batch) when `count` is given or
 * rows are merged; GBRS_EM_NO_INTERLEAVE / GBRS_EM_FORCE_INTERLEAVE select among those two. */
#define GBRS_EM_NO_INTERLEAVE 4u
#define GBRS_EM_FORCE_INTERLEAVE 8u
#define GBRS_EM_NO_STREAMS 16u
/* Bit-reproducible sums: the E-step's LDS float64 atomics are replaced by a fixed-order reduction
 * (every wavefront of a tile owns a private copy of the tile's partial sums; lanes that hand in sums
 * for one locus are added by a fixed tree; copies, slots and block sums are added in index order), so
 * two runs on the same input give bit-identical theta and therefore the same iteration count even when
 * err_sum lands next to 1e6*tol (EMfactory.py:266).  The tiles are cut smaller (at most
 * (4160/8 - 1)/H loci each); not available with GBRS_EM_LAYOUT_CSC or H > 16. */
#define GBRS_EM_DETERMINISTIC 32u
/* Keep the uploaded CSC arrays on the handle until gbrs_em_set_initial_values has run (files that
 * store alignment values other than 1). */
#define GBRS_EM_KEEP_CSC 64u
/* This handle is one of two locus ranges of one sample that run side by side on the device (the two engines of
 * a rank in gbrs_amd/dist.py PipelinedShardedEM): the layout sizes its tiles for the two together. */
#define GBRS_EM_SIDE_BY_SIDE 128u
/* The process builds this one handle and exits (the `gbrs quantify` command): the multi-gigabyte temporaries of the
 * layout build and the uploaded CSC copy stay allocated until gbrs_em_destroy instead of being freed when create
 * returns (on some hosts a hipMalloc that follows a large hipFree stalls for 0.1-0.2 s; the whole create is ~45 ms
 * shorter).  gbrs_em_info.retained_build_bytes reports what is held.  Without the flag create frees them in one pass
 * before it returns, so several live handles cost their layouts only. */
#define GBRS_EM_ONE_SHOT 256u
/* Locus sets off.  By default a read whose alignments to several loci all carry the same haplotype mask may be stored
 * as one word on the id of its locus SET: its denominator is sum_h m_h * (theta[l1,h] + theta[l2,h] + ...) and every
 * member locus receives the same count/den, so the set behaves like one locus whose theta is the sum of its members'.
 * The sets exist inside the tiles only (a tile sums the members' theta for a set entry and stores the entry's sums once
 * per member locus); theta, the expected counts and the M-step are per locus as before.  Same arithmetic up to the
 * association of those sums (agrees with the plain form to ~1e-15 relative).  The layout takes the sets when they
 * remove >= 15 % of the words, leave >= 100 words per id and number at most twice the loci, and never for weighted rows
 * (count given or identical rows merged); gbrs_em_info.num_locus_sets says how many it found (0: not taken).  The flag keeps one word per
 * (read, locus) pair whatever the sample. */
#define GBRS_EM_NO_LOCUS_SETS 512u
/* Multiread models 1-3 (EMfactory.py:160-203): the handle keeps the CSC row ids after create, so that
 * gbrs_em_set_groups can build the grouped row layout those models step on.  Model 4 is unaffected. */
#define GBRS_EM_GROUPED_MODELS 1024u
/* Read-level posteriors (gbrs_em_posterior).  The handle keeps the CSC row ids and column pointers after create
 * (after a `-G` mask; the arrays GBRS_EM_GROUPED_MODELS keeps, shared when both are set) and copies theta into a
 * second H*L buffer before every EM step: the theta that step's E-step used.  Without the flag a handle allocates
 * and launches exactly what it did before the flag existed. */
#define GBRS_EM_POSTERIOR 2048u
/* Bootstrap replicates (gbrs_em_resample).  The handle is built as a weighted one - base weights of `count`, or ones -
 * and keeps what it needs to write other row weights over them in place: the base count as integers and the file row
 * behind every word of the tiles and every long row.  GBRS_ERR_UNSUPPORTED with GBRS_EM_MERGE_IDENTICAL_ROWS or
 * GBRS_EM_SIDE_BY_SIDE; GBRS_ERR_INVALID for a count that is negative, not an integer or >= 2^32;
 * gbrs_em_set_initial_values on such a handle is GBRS_ERR_UNSUPPORTED.  On such a handle a row whose weight is 0 takes no
 * part: it adds nothing, and a zero denominator of its own is no float error.  Without the flag a handle allocates and
 * launches exactly what it did before the flag existed. */
#define GBRS_EM_RESAMPLE 4096u
/* Run words off.  By default reads that are ONE word in the tiles (one locus, or one locus set) and identical - same entry,
 * same haplotype mask - may share a word: each of them adds the same 1/den to its locus in every iteration, so the
 * word carries how many further reads it stands for (up to 1,023 at <= 8 haplotypes) and adds (1 + n)/den once.  Reads of
 * exactly TWO words that are identical pair for pair share their two words the same way (gbrs_em_fold_counts).  Nothing
 * becomes weighted and every read is counted; the result agrees with the one-word-per-read form up to the association of
 * the sums.  The layout takes the fold for unweighted stream-order handles of 1, 2, 4 or 8 haplotypes (never with `count`,
 * GBRS_EM_MERGE_IDENTICAL_ROWS, GBRS_EM_RESAMPLE or GBRS_EM_DETERMINISTIC) when it removes >= 15 % of the words and the words
 * left still give every resident workgroup place of the device a full tile; gbrs_em_info.num_folded_rows says how many
 * reads have no word of their own (0: not taken).  The flag keeps one word per read whatever the sample. */
#define GBRS_EM_NO_RUN_WORDS 8192u
/* `replicate` of gbrs_em_resample that puts the base weights back */
#define GBRS_RESAMPLE_BASE 0xFFFFFFFFu

/*
 * Replaces: AlignmentPropertyMatrix(h5file=...) as consumed by EMfactory.__init__
 * (emase/Sparse3DMatrix.py:80-92 CSC branch, emase/AlignmentPropertyMatrix.py:72-73 count,
 * emase/EMfactory.py:60-94 target_lengths).
 *
 *   num_rows  R reads / equivalence classes        num_loci  L isoforms      num_haps  H (<= 32)
 *   indptr[h]   uint32[L+1]  column pointers of haplotype h's (R x L) CSC incidence matrix
 *   indices[h]  uint32[nnz_h] row (read) ids, any order inside a column, no duplicates
 *   count       double[R] EC multiplicities, or NULL (every row counts once)
 *   eff_len     double[H*L] row-major max(len - read_length + 1, 1), or NULL (no length model)
 *   device      HIP device ordinal
 */
int gbrs_em_create(uint64_t num_rows, uint32_t num_loci, uint32_t num_haps,
                   const uint32_t *const *indptr, const uint32_t *const *indices,
                   const double *count, const double *eff_len,
                   int device, uint32_t flags, gbrs_em_t **out);

/* Same, but every array pointer (indptr[h], indices[h], count, eff_len) is a DEVICE pointer on
 * `device`; the pointer tables indptr/indices themselves are host arrays of H device pointers.
 * The inputs are only read during the call. */
int gbrs_em_create_device(uint64_t num_rows, uint32_t num_loci, uint32_t num_haps,
                          const uint32_t *const *indptr, const uint32_t *const *indices,
                          const double *count, const double *eff_len,
                          int device, uint32_t flags, gbrs_em_t **out);

/*
 * The same with the `-G` genotype mask of `gbrs quantify` applied on the device.  Replaces
 * gbrs/emase_utils.py:240-273: `aln_mat.multiply(gtmask, axis=2)` followed by `eliminate_zeros()` per haplotype,
 * i.e. every stored entry (h, l, r) whose haplotype h is not one of the two called for the gene of locus l leaves
 * the structure before EMfactory sees it (rows left without entries drop out, as they do there).
 *   allowed  HOST uint32[L] in both variants, bit h set = entries of (haplotype h, locus l) stay; NULL = no mask.
 * The mask selects whole CSC columns, so the library uploads the arrays as they are and moves the surviving
 * columns together on the device; no host pass over the entries.  gbrs_em_info.num_entries is the masked count;
 * values given to gbrs_em_set_initial_values still line up with the indices arrays as passed here.
 */
int gbrs_em_create_masked(uint64_t num_rows, uint32_t num_loci, uint32_t num_haps,
                          const uint32_t *const *indptr, const uint32_t *const *indices,
                          const double *count, const double *eff_len, const uint32_t *allowed,
                          int device, uint32_t flags, gbrs_em_t **out);
int gbrs_em_create_masked_device(uint64_t num_rows, uint32_t num_loci, uint32_t num_haps,
                                 const uint32_t *const *indptr, const uint32_t *const *indices,
                                 const double *count, const double *eff_len, const uint32_t *allowed,
                                 int device, uint32_t flags, gbrs_em_t **out);

/* Stored alignment values (an EMASE file saved with incidence_only = False, or a legacy COO file:
 * emase/Sparse3DMatrix.py:84-88, :93-99): values[h] double[nnz_h], aligned with indices[h] as given to
 * create.  EMfactory.prepare normalises them per read and that is all they are used for
 * (EMfactory.py:95-98; every E-step starts again from ones, Sparse3DMatrix.py:220-228), so this call
 * computes prepare()'s column sums from them once; prepare then uses those instead of 1/nnz_row.
 * Needs GBRS_EM_KEEP_CSC at create; call it once, before gbrs_em_prepare*. */
int gbrs_em_set_initial_values(gbrs_em_t *em, const double *const *values);

/* Replaces EMfactory.prepare (EMfactory.py:95-111): theta0 = sum_r count[r]/nnz_row / eff_len,
 * then the optional pseudocount rule (:105-111).  A handle without entries (empty columns, or a mask that
 * removes every entry) gets theta = 0 whatever the pseudocount - no locus has a value to add it to, and
 * there is no total to rescale to; a step or a run on it is GBRS_ERR_FLOAT, the reference's division by
 * the zero total. */
int gbrs_em_prepare(gbrs_em_t *em, double pseudocount);

/* n_iters EM steps (EMfactory.update_allelic_expression, EMfactory.py:214-232) without looking
 * at the stopping rule; err_sum_out (nullable) receives the last step's total TPM change. */
int gbrs_em_step(gbrs_em_t *em, int n_iters, double *err_sum_out);

/* Gene groups for multiread models 1-3 (handle created with GBRS_EM_GROUPED_MODELS, else GBRS_ERR_STATE).
 * group_ptr int64[G+1], members int64[..] locus ids, as for gbrs_em_group_sums; a locus in no group is a gene of
 * its own (EMfactory.py:48-59: t2t_mat is the identity there).  A locus in two groups is GBRS_ERR_INVALID.
 * Builds the grouped row layout on the device: every stored entry (after a `-G` mask) sorted by (read, gene,
 * locus, haplotype), or by (read, gene, haplotype, locus) for Model 1 (built at its first step). */
int gbrs_em_set_groups(gbrs_em_t *em, int64_t num_groups, const int64_t *group_ptr, const int64_t *members);

/* n_iters EM steps of multiread model `model` (1-4; 4 is gbrs_em_step).  With the factor
 *   f = 1 (model 4), T_g / S[r,g] (3), U_l T_g / (V[r,l] W[r,g]) (2), Y[h,g] T_g / (X[r,g,h] Z[r,g]) (1)
 * of a stored entry (read r, haplotype h, locus l in gene g) and D_r = sum of T_g over the genes read r touches,
 *   A[h,l] = sum_r count[r] f / D_r,  theta' = theta * A / len,  expected counts = theta * A,
 * where T_g, Y[h,g], U_l are gene, gene-haplotype and locus totals of theta and S, V, W, X, Z the sums of theta
 * over a read's entries of one gene / one locus, of U over the loci / of Y over the haplotypes a read touches in a
 * gene, of theta over a read's entries of one gene and haplotype.  An entry whose theta is 0 takes no
 * part (the reference eliminates zeros before each division).  Models 1-3 need gbrs_em_set_groups
 * (GBRS_ERR_UNSUPPORTED without it, or with GBRS_EM_DETERMINISTIC). */
int gbrs_em_step_model(gbrs_em_t *em, int model, int n_iters, double *err_sum_out);

/* Replaces EMfactory.run (EMfactory.py:234-287).  model 1-4 (1-3: see gbrs_em_step_model).  Stops when
 * err_sum <= 1e6*tol or after max_iters steps.  err_hist (nullable) receives up to
 * err_hist_cap per-iteration err_sum values (the numbers the reference prints); elapsed_s (nullable,
 * same capacity) the wall-clock seconds since the start of the run at which each iteration was
 * complete on the host's side - the "Time" column of the reference's progress table (:284-287).
 * The device loop hands control back once per batch of 8 iterations, so the iterations of a batch
 * share one time stamp. */
int gbrs_em_run(gbrs_em_t *em, int model, double tol, int max_iters,
                int *n_iters_out, double *err_hist, int err_hist_cap, double *elapsed_s);

/* theta (H x L) = EMfactory.allelic_expression; expected_counts (H x L) = probability.sum(READ)
 * of the last E-step (EMfactory.py:302), i.e. theta_before * A of the last iteration - on the single-GPU path formed
 * as theta * effective_length from the theta that iteration's M-step left (the same number up to two roundings), when
 * this call or gbrs_em_group_sums asks for it.  They stay those of the last iteration when gbrs_em_set_theta replaces
 * theta afterwards (the reports rescale theta to TPM first).  Either pointer may be NULL. */
int gbrs_em_get(gbrs_em_t *em, double *theta, double *expected_counts);

/* The posterior of every stored entry of haplotype `hap` in the most recent E-step (handle created with
 * GBRS_EM_POSTERIOR): what the reference's probability.data[hap] holds after a step.  out is a HOST array
 * double[nnz_hap], nnz_hap being the entries of the haplotype after a `-G` mask; the values come in the order of
 * the (masked) indices[hap] given to create: surviving columns in locus order, the entries of a column in the order
 * they were uploaded.  For an entry (read r, haplotype h, locus l) the value is theta_before[h,l] * f / D_r with f
 * and D_r as for gbrs_em_step_model, for whichever model (1-4) the last step ran and theta_before the theta that
 * step started from; `count` plays no part.  An entry whose theta_before is 0 gets exactly 0.0.  The result does
 * not depend on the layout the EM runs on.  The first call after a step computes the per-read denominators
 * (model 4) once; calls for the other haplotypes reuse them until the next step.  Models 1-3 divide the count back
 * out of the per-entry factors the step stored, so a read whose count is 0 has no defined posterior there (NaN).
 * GBRS_ERR_STATE without the flag or when no step has run since prepare; GBRS_ERR_INVALID for hap >= num_haps or
 * out_len != nnz_hap. */
int gbrs_em_posterior(gbrs_em_t *em, uint32_t hap, double *out, uint64_t out_len);

/* Bootstrap replicates (handle created with GBRS_EM_RESAMPLE, else GBRS_ERR_STATE).
 *   resample  draws the weights of replicate `replicate` on the device and installs them in every structure the handle
 *             steps on (tile words, long rows, the per-row array of the CSC, models 1-3 and posterior kernels - prepare
 *             uses the same).  Row r gets  w = sum_{k < c_r} P(u_k):  c_r = count[r] (1 without a count vector), u_k word
 *             k mod 4 of Philox4x32-10 with counter (r & 0xFFFFFFFF, r >> 32, k div 4, replicate) and key
 *             (seed & 0xFFFFFFFF, seed >> 32), P(u) = the number of j in 0..12 with u >= floor(2^32 sum_{i<=j} e^-1/i!):
 *             Poisson(c_r) by inversion, an integer, a function of (seed, replicate, r, c_r) alone - the same on every
 *             layout and under every `-G` mask.  A replicate is the quantification of the file in which row r occurs w
 *             times.  replicate == GBRS_RESAMPLE_BASE restores the base weights exactly.  The caller then runs
 *             gbrs_em_prepare and gbrs_em_run as on any handle.
 *   weights   the current weights in file row order, double[R] (rows a `-G` mask emptied included).
 *   resample_info   device bytes the flag added to the handle, rows whose count is above the cut (a workgroup each in
 *             the draw) and the cut (any pointer may be NULL). */
int gbrs_em_resample(gbrs_em_t *em, uint64_t seed, uint32_t replicate);
int gbrs_em_weights(gbrs_em_t *em, double *out);
int gbrs_em_resample_info(gbrs_em_t *em, uint64_t *extra_device_bytes, uint64_t *num_big_rows, uint32_t *cut);

/* Replicate statistics on the device (any handle).
 *   begin  clears them; groups as for gbrs_em_group_sums, num_groups = 0: isoform level only.
 *   add    folds the handle's current result in as one more replicate: TPM = theta * (1e6 / sum of theta), the expected
 *          read counts of the last E-step, their per-locus totals over the haplotypes, and with groups the same at gene
 *          level (the members' values added in member order).  Running mean and sum of squared deviations (Welford),
 *          updated in replicate order; every sum has a fixed order, so the statistics are bit-reproducible for a given
 *          sequence of thetas.  tpm, counts (H x L), gene_tpm, gene_counts (H x G), any nullable: the values of this
 *          replicate as they were folded in.
 *   get    level 0 isoforms / 1 genes (n = L / G): means and standard deviations with B - 1 in the denominator,
 *          (H x n) and, for the totals, n; any pointer may be NULL. */
int gbrs_em_bootstrap_begin(gbrs_em_t *em, int64_t num_groups, const int64_t *group_ptr, const int64_t *members);
int gbrs_em_bootstrap_add(gbrs_em_t *em, double *tpm, double *counts, double *gene_tpm, double *gene_counts);
int gbrs_em_bootstrap_get(gbrs_em_t *em, int level, uint32_t *num_replicates, double *tpm_mean, double *tpm_sd,
                          double *count_mean, double *count_sd, double *tpm_total_mean, double *tpm_total_sd,
                          double *count_total_mean, double *count_total_sd);

/* Overwrite theta (H x L), e.g. to resume from a checkpoint. */
int gbrs_em_set_theta(gbrs_em_t *em, const double *theta);

/* Gene-level sums: EMfactory.get_allelic_expression(at_group_level=True) (EMfactory.py:140-142)
 * and the grp_wise branch of report_read_counts (:305).  group_ptr int64[G+1], members int64[..]
 * locus ids.  which: 0 = theta, 1 = expected counts.  out is (H x G) row-major. */
int gbrs_em_group_sums(gbrs_em_t *em, int64_t num_groups, const int64_t *group_ptr,
                       const int64_t *members, int which, double *out);

/* Multi-GPU building blocks (rows sharded across ranks): one E-step over this
 * handle's rows accumulated into the handle's own partial buffer; the caller all-reduces that
 * buffer (RCCL) and then finishes the step.  partial_dev returns the DEVICE pointer of the
 * (L x H, locus-major) float64 partial-sum buffer and its element count. */
int gbrs_em_estep_partial(gbrs_em_t *em, void **partial_dev, uint64_t *n_elems);
/* M-step + stopping-rule bookkeeping on the all-reduced buffer.  With err_sum_out == NULL the error
 * pass (sum |dTPM|, iteration counter) is deferred into the next E-step launch; it is completed by
 * the next call that reports it (gbrs_em_finish_step with err_sum_out, gbrs_em_step, gbrs_em_sync). */
int gbrs_em_finish_step(gbrs_em_t *em, double *err_sum_out);
/* Same pair for prepare(): partial sums of count/nnz_row, then the division and pseudocount. */
int gbrs_em_prepare_partial(gbrs_em_t *em, void **partial_dev, uint64_t *n_elems);
int gbrs_em_finish_prepare(gbrs_em_t *em, double pseudocount);
/* The HIP stream (hipStream_t) the handle launches on, so the caller can order a collective. */
void *gbrs_em_stream(gbrs_em_t *em);
/* Launch on the caller's stream instead (e.g. torch's current stream, so that an RCCL all-reduce
 * issued through torch.distributed is ordered with the E-step without host synchronisation).
 * The caller keeps ownership of the stream. */
int gbrs_em_set_stream(gbrs_em_t *em, void *stream);
int gbrs_em_sync(gbrs_em_t *em);

/* Two handles that hold the two locus ranges of ONE sample (cut where no row straddles, GBRS_EM_SIDE_BY_SIDE; the two
 * engines of a rank in gbrs_amd/dist.py PipelinedShardedEM) share only the stopping rule of EMfactory.run
 * (emase/EMfactory.py:266-278): err_sum runs over the loci of both, scaled by the totals of both.  These calls evaluate
 * it on the device, with no host synchronisation in the loop, so that the pair stops at the reference's iteration:
 *   pair_begin   clears both handles' step scalars and the pair's counters (max_iters sizes the error history)
 *   pair_check   after gbrs_em_finish_step of BOTH handles for an iteration (a's first): enqueues the rule on b's
 *                stream behind a's M-step; when err_sum <= 1e6 * tol it raises both handles' stop flags - every later
 *                kernel of either is a no-op, theta stays the stopping iteration's; a's next M-step waits for it
 *   pair_status  synchronises and returns the iterations applied, the stop flag and the err_sum sequence */
int gbrs_em_pair_begin(gbrs_em_t *a, gbrs_em_t *b, int max_iters);
int gbrs_em_pair_check(gbrs_em_t *a, gbrs_em_t *b, double tol);
int gbrs_em_pair_status(gbrs_em_t *a, gbrs_em_t *b, int *iters_done, int *stopped, double *err_hist, int err_hist_cap);

typedef struct gbrs_em_info {
    uint64_t num_rows;          /* R as given                                               */
    uint64_t num_entries;       /* N = sum_h nnz_h                                          */
    uint64_t num_device_rows;   /* reads the device layout represents (== R unless merged)  */
    uint64_t num_device_words;  /* 32-bit (row, locus) words streamed per E-step            */
    uint64_t bytes_per_iter;    /* bytes the E+M step kernels move per iteration (layout)   */
    uint64_t algorithmic_bytes; /* 4N + 4(R+1) [+8R] + 8HL*2 [+8HL]             */
    double   last_estep_ms;     /* HIP-event time of the E-step launch (mean of the timed    */
    double   last_step_ms;      /* steps: every 8th of a gbrs_em_step call) / of a full step.
                                   On the gather-side route (gbrs_em_gather_mstep) a step IS its one
                                   launch: last_estep_ms is that launch, last_step_ms the same     */
    uint32_t num_loci, num_haps;
    uint32_t layout;            /* 0 = csc-direct, 1 = packed row tiles                     */
    uint32_t num_folded_rows;   /* layout 1: one-word reads counted by an identical read's word instead of a word of
                                   their own (two-word reads: gbrs_em_fold_counts); 0: the fold was not taken
                                   (GBRS_EM_NO_RUN_WORDS).  The slot was
                                   `reserved` (always 0): the struct keeps its size and offsets; the tile layout
                                   holds fewer than 2^32 entries, so 32 bits do                        */
    uint64_t num_tiles;         /* layout 1: workgroup tiles                                */
    uint64_t num_slots;         /* layout 1: (tile, locus) partial-sum slots                */
    uint64_t num_long_rows;     /* layout 1: rows handled by the long-row kernel            */
    uint64_t num_heavy_loci;    /* layout 1: loci with more than 16 slots (one wavefront each in the
                                   gather: emase/AlignmentPropertyMatrix.py:288-298 column sums)   */
    uint64_t num_light_loci;    /* layout 1: loci with 2..16 slots (summed in place)        */
    uint64_t estep_bytes;       /* bytes the E-step kernel itself moves per launch: word stream, tile
                                   headers, dictionary, theta gather, slot stores [, row weights]  */
    uint64_t retained_build_bytes; /* device bytes of build temporaries the handle still holds
                                   (GBRS_EM_ONE_SHOT; 0 otherwise)                                */
    uint64_t num_locus_sets;       /* distinct locus sets of the tile layout (GBRS_EM_NO_LOCUS_SETS: 0) */
} gbrs_em_info_t;
int gbrs_em_info(gbrs_em_t *em, gbrs_em_info_t *info);
/* Reads without words of their own in the tile layout, by kind: one_word_reads is gbrs_em_info.num_folded_rows (reads of one
 * locus or one locus set counted by an identical read's word); two_word_reads are reads of exactly two (locus, mask) pairs
 * counted by an identical read's two words.  Both 0 when the fold was not taken and for the CSC layout. */
int gbrs_em_fold_counts(gbrs_em_t *em, uint64_t *one_word_reads, uint64_t *two_word_reads);
/* How the tile layout was cut.  passes: the passes of the exact cut - a tile ends at tile_words words or at its dictionary's
 * capacity in DISTINCT ids, and the size is rescaled towards one round of the device's workgroup places - or 0 for the
 * two-grid cut (GBRS_TUNING_TILE_WORDS forces the size, or GBRS_TUNING_TILE_CUT=0); tile_words: the size that cut the
 * tiles.  Both 0 for the CSC layout. */
int gbrs_em_tile_cut(gbrs_em_t *em, uint32_t *passes, uint32_t *tile_words);
/* Do the handle's Model-4 steps (gbrs_em_step, gbrs_em_run), as it stands, take the gather-side M-step: iteration n's
 * M-step applied by the tile prologues of launch n + 1, one launch per iteration and one elementwise M-step at the end of a
 * call?  taken: 1 / 0 (GBRS_TUNING_NO_GATHER_MSTEP=1 at create, heavy loci, long rows, weights, the deterministic mode,
 * 16 haplotypes, posteriors, resampling, pair mode or a handed-out acc: 0). */
int gbrs_em_gather_mstep(gbrs_em_t *em, uint32_t *taken);
/* Per tile, in launch order: its batches of 64 words and its dictionary entries.  n must be gbrs_em_info.num_tiles; one
 * device-to-host copy of the headers (profiling scripts and tests). */
int gbrs_em_tile_shapes(gbrs_em_t *em, uint32_t *n_batches, uint32_t *dict_entries, uint64_t n);
/* How often the lanes of a wavefront change dictionary entry in the tiles' counted batches (the leading runs of one-word
 * rows and of two-word rows; GBRS_TUNING_STRIPES lays their groups out in stripes of S cells).  A host walk over a copy of
 * the headers and words, batch by batch as the E-step's wavefronts take them: wavefront w of a tile has batches
 * [nb w / 8, nb (w + 1) / 8) and starts on no entry.  out[0] counted batches; out[1] the wavefronts' first batches among
 * them; out[2] later batches in which at least one lane's dictionary index differs from the cell above it; out[3] the
 * lanes that change in those; out[4] cells of counted batches without a haplotype bit (padding); out[5] the batches of
 * out[2] that are not a multiple of S from their run's first batch (S = 0: 0).  All 0 for the CSC layout.  Off the hot
 * path (profiling scripts and tests). */
int gbrs_em_stripe_census(gbrs_em_t *em, uint32_t S, uint64_t *out);

/* `--report-alignment-counts` (emase/AlignmentPropertyMatrix.py:389-459), stand-alone (the
 * reference reloads the alignment file for it, gbrs/emase_utils.py:318-331).  Inputs as for
 * gbrs_em_create.  locus_group (nullable) int32[L] maps every locus to an output column, which
 * gives the gene-level report after _bundle_inline(reset=True) (:155-188); -1 = the locus is in no
 * group: its entries drop out, as they do from the product with grp_conv_mat.  num_out_loci = G
 * then, ignored (= L) otherwise.  Outputs, any nullable: aln_counts and allele_unique (H x Lout)
 * row-major, locus_unique (Lout).  Sums of EC counts in float64: exact for integer counts. */
int gbrs_alignment_counts(uint64_t num_rows, uint32_t num_loci, uint32_t num_haps,
                          const uint32_t *const *indptr, const uint32_t *const *indices,
                          const double *count, const int32_t *locus_group, uint32_t num_out_loci,
                          int device, double *aln_counts, double *allele_unique, double *locus_unique);

/* The same in three calls, for callers that want both levels (the `quantify -a` command writes the isoform-level and
 * the gene-level report, AlignmentPropertyMatrix.py:442-459 twice): create uploads the alignments once, every get
 * computes one set of counts (locus_group / num_out_loci as above) and re-uses the device workspace of the last. */
typedef struct gbrs_counts gbrs_counts_t;
int gbrs_counts_create(uint64_t num_rows, uint32_t num_loci, uint32_t num_haps,
                       const uint32_t *const *indptr, const uint32_t *const *indices,
                       const double *count, int device, gbrs_counts_t **out);
int gbrs_counts_get(gbrs_counts_t *c, const int32_t *locus_group, uint32_t num_out_loci,
                    double *aln_counts, double *allele_unique, double *locus_unique);
int gbrs_counts_destroy(gbrs_counts_t *c);

/* ------------------------------------------------------------------------------------------
 * Row sharding of one sample over N ranks (`gbrs quantify --gpus N`), on the device.
 * indptr / indices are host tables of H DEVICE pointers to the sample's CSC arrays (as for
 * gbrs_em_create_device); every result equals gbrs_amd.dist.shard_rows bit for bit.  The calls
 * are synchronous.  A row id >= num_rows or a malformed column pointer table is GBRS_ERR_INVALID.
 * ---------------------------------------------------------------------------------------- */
/* bounds (host uint64[world + 1]): row blocks balanced by entry count, bounds[k] =
 * searchsorted(cum, total * k / world, 'left') over the per-row entry counts (cum[0] = 0),
 * bounds[0] = 0, bounds[world] = num_rows.  1 <= world <= 64. */
int gbrs_shard_plan(uint64_t num_rows, uint32_t num_loci, uint32_t num_haps,
                    const uint32_t *const *indptr, const uint32_t *const *indices,
                    int world, int device, uint64_t *bounds);
/* Column pointers of the rows [r0, r1): indptr_out[h] device uint32[L + 1] (caller-allocated);
 * nnz_out (host uint64[H]) the entries kept per haplotype. */
int gbrs_shard_index(uint64_t num_rows, uint32_t num_loci, uint32_t num_haps,
                     const uint32_t *const *indptr, const uint32_t *const *indices,
                     uint64_t r0, uint64_t r1, int device,
                     uint32_t *const *indptr_out, uint64_t *nnz_out);
/* The kept entries of the rows [r0, r1): indices_out[h] device uint32[nnz_local[h]] with row ids
 * re-based to r0 (column order kept) and, when values (device double tables aligned with indices)
 * is not NULL, values_out[h] device double[nnz_local[h]].  nnz_local (host) is what
 * gbrs_shard_index reported; a mismatch is GBRS_ERR_INVALID and nothing is written.
 * l_split in (0, L): *straddling = the number of local rows with entries in loci on both sides
 * of l_split; l_split = 0: not asked (straddling may be NULL). */
int gbrs_shard_gather(uint64_t num_rows, uint32_t num_loci, uint32_t num_haps,
                      const uint32_t *const *indptr, const uint32_t *const *indices,
                      uint64_t r0, uint64_t r1, uint32_t l_split, const double *const *values,
                      int device, const uint64_t *nnz_local, uint32_t *const *indices_out,
                      double *const *values_out, uint64_t *straddling);

int gbrs_em_destroy(gbrs_em_t *em);

/* `gbrs compress` numeric body (gbrs/emase_utils.py:60-103): rows with identical alignment patterns
 * collapse into equivalence classes (ECs) whose count is the sum of the member counts; classes are
 * numbered in order of first appearance (the reference's dict insertion order, :77/:95); rows
 * without any alignment form one class with the empty key, as they do there.  Inputs as for
 * gbrs_em_create (several files = their rows concatenated by the caller).  create returns the
 * number of classes and the entries per haplotype so that the caller can size the outputs of get:
 * indptr_out[h] uint32[L+1], indices_out[h] uint32[nnz_per_hap[h]] (class ids ascending inside a
 * column), count_out double[num_ecs]. */
typedef struct gbrs_compress gbrs_compress_t;
int gbrs_compress_create(uint64_t num_rows, uint32_t num_loci, uint32_t num_haps,
                         const uint32_t *const *indptr, const uint32_t *const *indices,
                         const double *count, int device, gbrs_compress_t **out,
                         uint64_t *num_ecs, uint64_t *nnz_per_hap);
int gbrs_compress_get(gbrs_compress_t *c, uint32_t *const *indptr_out, uint32_t *const *indices_out,
                      double *count_out);
int gbrs_compress_destroy(gbrs_compress_t *c);

/* Structure edits of one sample's incidence tensor, resident on the device: the numeric bodies of
 * `get-common-alignments` (emase/emase_utils.py:236-274 with Sparse3DMatrix.__mul__, Sparse3DMatrix.py:168-180),
 * `combine` (emase_utils.py:73-111, Sparse3DMatrix.py:383-398, AlignmentPropertyMatrix.py:461-476),
 * `pull-out-unique-reads` (emase_utils.py:277-317, AlignmentPropertyMatrix.py:372-413) and `stencil`
 * (gbrs/emase_utils.py:110-177: `multiply(gtmask, axis=2)` + `eliminate_zeros()`, saved instead of quantified).
 * Only the structure is held (every stored entry counts as present, whatever its value).
 *   create            uploads the arrays (as for gbrs_em_create: any order inside a column, no duplicates).
 *   intersect         m := the entries of m that b holds too (b: host arrays of the same R, L, H) - the elementwise
 *                     product of two incidence tensors.
 *   append_rows       m := the rows of m, then the num_rows_b rows of b (their ids shifted by R of m); R grows.
 *   keep_unique_rows  drops every entry of a row that is not unique.  A row is unique when all its entries carry one
 *                     key: the locus for ignore_haplotype != 0 (nnz of the haplotype sum == 1,
 *                     AlignmentPropertyMatrix.py:398-403), (haplotype, locus) otherwise (exactly one alignment,
 *                     :405-410).  With locus_group (int32[L], -1 = in no group; num_groups = G) the locus is replaced
 *                     by its group - the test on the matrix after bundle(reset=True) - entries of loci in no group
 *                     take no part in it, and the filter is applied to the isoform-level entries
 *                     (pull_alignments_from on the original matrix, emase_utils.py:299-308).  A row without any
 *                     counted entry is not unique.  keep_out (nullable) uint8[R]: 1 = the row stayed.
 *   mask_columns      drops the columns (h, l) with bit h of allowed[l] clear (allowed: host uint32[L]), what
 *                     gbrs_em_create_masked does before the EM.
 *   sizes / get       R, the entries per haplotype, and sorted_inputs = how many haplotype arrays given so far did not
 *                     have ascending columns and went through the radix sort (any pointer may be NULL);
 *                     indptr_out[h] uint32[L + 1], indices_out[h] uint32[nnz_per_hap[h]].
 * Every operand's row ids are range-checked on the device before a kernel indexes with them and its column pointer
 * tables are checked on the host (GBRS_ERR_INVALID); the row ids of every result ascend inside every column (what
 * scipy returns for the four operations); 2^32 or more rows, or entries of one haplotype, is GBRS_ERR_UNSUPPORTED;
 * there is no CPU fallback (GBRS_ERR_NO_DEVICE).  After a failed edit the handle is only good for destroy.
 *
 * `count-shared-multireads-pairwise` (emase/emase_utils.py:142-176: `hapsum.T * hapsum` with the stored values set to
 * one) reads the tensor and leaves it untouched:
 *   shared_counts      C = P^T P for the tensor as it stands, P the R x n pattern matrix: P[r, c] = 1 when row r has a
 *                      stored entry at column c in any haplotype.  locus_group NULL: n = L, a column is a locus.
 *                      Otherwise (int32[L], -1 = in no group; num_groups = G >= 1) n = G, a column is a group - the
 *                      matrix after _bundle_inline(reset=True) - and entries of loci in no group drop out.  C[i][i] is
 *                      the number of rows at column i, C[i][j] the number of rows at both.  Every row counts once.
 *                      The result stays on the device until the next shared_counts call or destroy; nnz_out
 *                      (nullable) receives its number of stored entries.  Counts are added up as 32-bit integers (a
 *                      count is at most R < 2^32) without atomics: exact, and identical from run to run.
 *   shared_counts_get  the result as CSR with both triangles, the column ids ascending inside every row and no stored
 *                      zero: indptr_out uint64[n + 1], indices_out uint32[nnz], data_out double[nnz].
 *   shared_counts_info how the last shared_counts call went (any pointer may be NULL): n, the distinct (row, column)
 *                      entries of P, the pairs (i <= j) emitted, the batches they were emitted and reduced in, the pair
 *                      budget of a batch, the peak of device bytes the call held (sampled after its large allocations)
 *                      and the milliseconds between its first and last device operation.
 * The pairs of all rows form one index space that is cut into batches of at most `budget` pairs, so the memory is
 * bounded whatever the sample and a single row with more pairs than the budget is split like any other stretch.  The
 * budget is 1/64 of the free device memory, in pairs, between 2^20 and 2^31; GBRS_SHARED_PAIR_BUDGET=<pairs> overrides
 * it (GBRS_ERR_INVALID when it is not a positive integer).  get and info before any shared_counts: GBRS_ERR_INVALID. */
typedef struct gbrs_matops gbrs_matops_t;
int gbrs_matops_create(uint64_t num_rows, uint32_t num_loci, uint32_t num_haps, const uint32_t *const *indptr,
                       const uint32_t *const *indices, int device, gbrs_matops_t **out);
int gbrs_matops_intersect(gbrs_matops_t *m, const uint32_t *const *indptr_b, const uint32_t *const *indices_b);
int gbrs_matops_append_rows(gbrs_matops_t *m, uint64_t num_rows_b, const uint32_t *const *indptr_b,
                            const uint32_t *const *indices_b);
int gbrs_matops_keep_unique_rows(gbrs_matops_t *m, const int32_t *locus_group, uint32_t num_groups,
                                 int ignore_haplotype, uint8_t *keep_out);
int gbrs_matops_mask_columns(gbrs_matops_t *m, const uint32_t *allowed);
int gbrs_matops_sizes(gbrs_matops_t *m, uint64_t *num_rows, uint64_t *nnz_per_hap, uint32_t *sorted_inputs);
int gbrs_matops_get(gbrs_matops_t *m, uint32_t *const *indptr_out, uint32_t *const *indices_out);
int gbrs_matops_shared_counts(gbrs_matops_t *m, const int32_t *locus_group, uint32_t num_groups, uint64_t *nnz_out);
int gbrs_matops_shared_counts_get(gbrs_matops_t *m, uint64_t *indptr_out, uint32_t *indices_out, double *data_out);
int gbrs_matops_shared_counts_info(gbrs_matops_t *m, uint64_t *num_columns, uint64_t *pattern_entries,
                                   uint64_t *pairs_emitted, uint32_t *batches, uint64_t *pair_budget,
                                   uint64_t *peak_device_bytes, double *device_ms);
int gbrs_matops_destroy(gbrs_matops_t *m);

/* The alignment tensor with values, and the arithmetic the reference builds every model from (emase/Sparse3DMatrix.py
 * reset :220-228, multiply :314-377, copy; emase/AlignmentPropertyMatrix.py sum :275-303, normalize_reads :305-370).
 * A tensor is the stored entries (read r, haplotype h, locus l) of the per-haplotype CSC arrays with one double each,
 * `count` (nullable) and gene groups (optional).  The structure never changes after create; copy() shares it by reference
 * count, so a handle and its copies may be destroyed in any order.  They also share one stream and the structure's
 * scratch buffers: drive a tensor and its copies from one thread.
 *   create      values: NULL (every entry 1) or H pointers, values[h] lined up with indices[h].  Row ids are checked
 *               against num_rows.  GBRS_ERR_UNSUPPORTED with 2^32 - 1 or more entries or 2^27 or more loci.
 *   set_groups  the genes of normalize(GROUP | HAPLOGROUP): the groups, then every locus in no group as a gene of its own
 *               (validation and messages as gbrs_em_set_groups).  Without the call every locus is a gene of its own.  The
 *               genes belong to the structure: they change for every copy.
 *   reset       v = 1
 *   multiply    form 1: v *= m[l], m_len = L           (multiplier 1-D, axis 1)
 *               form 2: v *= m[r], m_len = R           (1-D, axis 2)
 *               form 3: v *= m[r*H + h], m_len = R*H   (2-D dense R x H, axis 0)
 *               form 4: v *= m[h*L + l], m_len = H*L   (2-D H x L, axis 2)
 *               m is a host array; any other form or length is GBRS_ERR_INVALID.
 *   multiply_tensor   v *= other's v; other must share t's structure (t itself or a copy), else GBRS_ERR_UNSUPPORTED
 *   normalize   axis 0 LOCUS, 1 HAPLOTYPE, 2 READ, 3 GROUP, 4 HAPLOGROUP: v /= the sum over the read's entries of the same
 *               locus / haplotype / read / gene / gene and haplotype.  LOCUS, GROUP and HAPLOGROUP first eliminate every
 *               entry whose value is 0 (the reference's eliminate_zeros()): it keeps 0 through every later operation,
 *               reset included, and no longer counts in nnz.  A live entry over a zero sum is left unchanged and the call
 *               returns GBRS_ERR_FLOAT after the other reads have been normalised.
 *   sum_reads   out (H x L) = sum over the reads of count[r] * v (count 1 when absent).  Float atomics: the last bits
 *               depend on the order of arrival.  Every other operation here is bit-identical from run to run.
 *   sum_loci    out (R x H) = sum over the loci of v
 *   values / set_values   one haplotype's values in the order of indices[h] (len = its number of stored entries);
 *               live (nullable, uint8) = 1 where the entry is not eliminated.  set_values leaves eliminated entries 0.
 *   nnz         live entries per haplotype, uint64[H] */
typedef struct gbrs_tensor gbrs_tensor_t;
int gbrs_tensor_create(uint64_t num_rows, uint32_t num_loci, uint32_t num_haps, const uint32_t *const *indptr,
                       const uint32_t *const *indices, const double *const *values /* nullable: ones */,
                       const double *count /* nullable */, int device, gbrs_tensor_t **out);
int gbrs_tensor_set_groups(gbrs_tensor_t *t, int64_t num_groups, const int64_t *group_ptr, const int64_t *members);
int gbrs_tensor_reset(gbrs_tensor_t *t);
int gbrs_tensor_multiply(gbrs_tensor_t *t, int form, const double *m, uint64_t m_len);
int gbrs_tensor_multiply_tensor(gbrs_tensor_t *t, const gbrs_tensor_t *other);
int gbrs_tensor_normalize(gbrs_tensor_t *t, int axis);
int gbrs_tensor_sum_reads(gbrs_tensor_t *t, double *out_HxL);
int gbrs_tensor_sum_loci(gbrs_tensor_t *t, double *out_RxH);
int gbrs_tensor_copy(gbrs_tensor_t *t, gbrs_tensor_t **out);
int gbrs_tensor_values(gbrs_tensor_t *t, uint32_t hap, double *out, uint8_t *live /* nullable */, uint64_t len);
int gbrs_tensor_set_values(gbrs_tensor_t *t, uint32_t hap, const double *v, uint64_t len);
int gbrs_tensor_nnz(gbrs_tensor_t *t, uint64_t *per_hap);
int gbrs_tensor_destroy(gbrs_tensor_t *t);

/* `gbrs bam2emase` (emase/AlignmentMatrixFactory.py:26-142): a BAM file -> the per-haplotype CSC incidence
 * matrices of the EMASE format plus the sorted distinct read names.
 *   open       reads the BGZF/BAM header (host only).  n_ref / ref_names_len size the buffers of
 *              gbrs_bam_references: the names one after another without terminators, name k at
 *              names[name_off[k] .. name_off[k+1]), name_off uint64[n_ref + 1], ref_len uint32[n_ref] or NULL.
 *              threads <= 0: GBRS_IO_THREADS or the machine's count; never more than 16 inflate threads.
 *   set_reference_map   hap[k], locus[k] of reference sequence k, as the caller split its name; a sequence no
 *              kept record may use has hap[k] = 0xFFFFFFFF and locus[k] = the reason: 1 the name does not split
 *              into (locus, haplotype), 2 unknown haplotype, 3 unknown locus.
 *   convert    one pass over the file on the host (inflate + parse; per record only the name, refID and flag
 *              are looked at), then on the device: rank the distinct names of ALL records bytewise (= the
 *              order of Python's sorted() for ASCII names), read id = rank; every record whose flag word is
 *              neither exactly 4 nor exactly 8 (an equality test, as in the reference, not a bit test) gives
 *              the entry (read id, locus) of its haplotype; duplicates are stored once.  The first such record
 *              without a reference sequence or with an unusable one is GBRS_ERR_INVALID, its sequence named in
 *              the message.  Out: num_reads, name_width (longest name, at least 1), nnz_per_hap uint64[H],
 *              stage_seconds double[3] (read, rank, build; NULL allowed).  GBRS_ERR_NO_DEVICE without a
 *              device - there is no CPU fallback; GBRS_ERR_UNSUPPORTED when 2^32 or more reads or entries of
 *              one haplotype, or when (haplotype, locus, read id) does not fit 64 bits.
 *   get        indptr_out[h] uint32[L + 1], indices_out[h] uint32[nnz_per_hap[h]] (read ids ascending inside a
 *              column), rname_out char[num_reads * name_width] zero padded (NULL to skip).
 *   scan_records   host only, for small files and tests: refID, flag and name of every record in file order.
 *              Arrays of `cap` entries (name_off: cap + 1), names as in gbrs_bam_references; n_records and
 *              names_len report the full sizes, so a first call with cap = 0 sizes the second. */
typedef struct gbrs_bam gbrs_bam_t;
int gbrs_bam_open(const char *path, int32_t threads, gbrs_bam_t **out, uint64_t *n_ref, uint64_t *ref_names_len);
int gbrs_bam_references(gbrs_bam_t *b, char *names, uint64_t names_cap, uint64_t *name_off, uint32_t *ref_len);
int gbrs_bam_set_reference_map(gbrs_bam_t *b, uint64_t n_ref, const uint32_t *hap, const uint32_t *locus,
                               uint32_t num_haps, uint32_t num_loci);
int gbrs_bam_convert(gbrs_bam_t *b, int device, uint64_t *num_reads, uint32_t *name_width, uint64_t *nnz_per_hap,
                     double *stage_seconds);
int gbrs_bam_get(gbrs_bam_t *b, uint32_t *const *indptr_out, uint32_t *const *indices_out, char *rname_out);
int gbrs_bam_scan_records(gbrs_bam_t *b, uint64_t cap, int32_t *refid, uint32_t *flag, uint64_t *name_off, char *names,
                          uint64_t names_cap, uint64_t *n_records, uint64_t *names_len);
int gbrs_bam_destroy(gbrs_bam_t *b);

/* `gbrs bam2ec` (extension): one or more BAM files -> the equivalence classes `gbrs bam2emase` on every file followed
 * by `gbrs compress -i f1 -i f2 ...` gives, without the read-level matrices or the read names leaving the device.
 *   create     an empty set for num_loci x num_haps (1 <= H <= 16, L < 2^27: the limits of compress).
 *   add_bam    b: opened, its reference map set with the same L and H (else GBRS_ERR_INVALID; no map: GBRS_ERR_STATE).
 *              Reads the file and ranks its names as convert does, builds the file's classes from the resident CSC
 *              arrays, and appends the file's reads after those already in the set: classes stay in first-occurrence
 *              order over all reads added so far, counts are numbers of reads, reads without a kept record form the
 *              empty class.  The same name in two files is two reads.  num_reads_of_file = 0 (and an unchanged set)
 *              for a file without any record.  stage_seconds double[3]: read, rank, classes (NULL allowed).  Record
 *              errors as for convert.  After a failure the set holds what it held before.  The bam handle keeps
 *              nothing on the device.
 *   add_bam_pair   the two ends of a paired-end sample, aligned one end at a time: adds what bam2emase on each end,
 *              `get-common-alignments -i first -i second` and compress give.  Both handles as for add_bam (same statuses).
 *              Each end's read ids are the ranks of its own distinct names; the two sorted name arrays must be equal
 *              byte for byte, else GBRS_ERR_INVALID with a message that starts "The read ID's are not compatible." and
 *              goes on to the first sorted position at which they differ, the name there and the file it is from (one
 *              end without any record against one with records is incompatible as well).  An entry (haplotype, locus,
 *              read) is kept iff both ends have it; a read left without entries is a read of the empty class.
 *              num_reads_of_pair = 0 and an unchanged set when neither file holds a record.  stage_seconds double[4]:
 *              read, rank, common (name check + intersection), classes (NULL allowed).  Record errors name the
 *              offending file.  After a failure the set holds what it held before; the handles keep nothing on the
 *              device.  add_bam and add_bam_pair may be mixed on one set.
 *   sizes      reads added, classes, entries per haplotype (uint64[H]); all zero for an empty set.
 *   get        indptr_out[h] uint32[L + 1], indices_out[h] uint32[nnz_per_hap[h]] (class ids ascending inside a
 *              column), count_out double[num_ecs] (NULL to skip).  An empty set has zero classes. */
typedef struct gbrs_ecset gbrs_ecset_t;
int gbrs_ecset_create(uint32_t num_loci, uint32_t num_haps, int device, gbrs_ecset_t **out);
int gbrs_ecset_add_bam(gbrs_ecset_t *e, gbrs_bam_t *b, uint64_t *num_reads_of_file, double *stage_seconds);
int gbrs_ecset_add_bam_pair(gbrs_ecset_t *e, gbrs_bam_t *first, gbrs_bam_t *second, uint64_t *num_reads_of_pair,
                            double *stage_seconds);
int gbrs_ecset_sizes(gbrs_ecset_t *e, uint64_t *num_reads, uint64_t *num_ecs, uint64_t *nnz_per_hap);
int gbrs_ecset_get(gbrs_ecset_t *e, uint32_t *const *indptr_out, uint32_t *const *indices_out, double *count_out);
int gbrs_ecset_destroy(gbrs_ecset_t *e);

/* ------------------------------------------------------------------------------------------
 * HMM: per-chromosome forward-backward + Viterbi over the S = H(H+1)/2 diplotype states.
 * ---------------------------------------------------------------------------------------- */

typedef struct gbrs_hmm gbrs_hmm_t;

/*
 * Replaces the `tprob = np.load(tprob_file)` tables as consumed by gbrs_utils.py:500-599.
 *   n_genes[c]  genes on chromosome c (genome order)       n_trans[c]  len(tprob[c])
 *   tprob[c]    double[n_trans[c]][S][S], natural-log, T[i][to][from], C order
 * n_trans[c] may be n_genes[c]-1 (tables written by get_transition_prob, gbrs_utils.py:273-278)
 * or >= n_genes[c] (DO tables); both backtrace conventions of gbrs_utils.py:589-596 are kept.
 */
int gbrs_hmm_create(int num_haps, int n_chrom, const int32_t *n_genes, const int32_t *n_trans,
                    const double *const *tprob, int device, gbrs_hmm_t **out);

/* Emission model on the device: gbrs_utils.py:463-492 with get_genotype_probability (:80-98).
 *   expr[c]     double[n_samples][n_genes[c]][H]   gene-level TPM per haplotype
 *   avecs[c]    double[n_genes[c]][H][H]           alignment specificity (row i = haplotype i)
 *   has_avec[c] uint8[n_genes[c]]  0 -> naive avecs with sigma fixed 0.450 (:483-487)
 * avecs / has_avec are sample independent: they are copied to the device when given and stay resident
 * on the handle, so later calls (the next sample or batch of samples) may pass NULL for both and move
 * only the expression rows.
 */
int gbrs_hmm_set_expression(gbrs_hmm_t *hmm, int n_samples, const double *const *expr,
                            const double *const *avecs, const uint8_t *const *has_avec,
                            double expr_threshold, double sigma);

/* Alternative to set_expression: caller-computed log emissions eprob[c] double[n_samples][n_c][S]. */
int gbrs_hmm_set_eprob(gbrs_hmm_t *hmm, int n_samples, const double *const *eprob);

/* forward (:500-526) + Viterbi delta/backpointers (:567-579), backward + posterior (:530-560),
 * backtrace (:580-598) for every (sample, chromosome). */
int gbrs_hmm_run(gbrs_hmm_t *hmm);

/* Results of one (sample, chromosome).  Every pointer is nullable.
 *   gamma  double[S][n_c]  C order, as saved in genoprobs.npz (gbrs_utils.py:558-563)
 *   states int32[n'+1]     ordered Viterbi path as saved in genotypes.npz, n' = min(n_c, n_trans)
 *   calls  int32[n_c]      state index written to genotypes.tsv per gene, -1 = no entry
 *   alpha, beta, delta  double[S][n_c];  scaler double[n_c];  eprob double[n_c][S]
 * alpha, scaler and beta are the reference's log-domain intermediates; gbrs reconstruct saves none of
 * them, so gbrs_hmm_run leaves them out and the first get that asks for one makes them for the
 * whole last run (one extra device pass). */
int gbrs_hmm_get(gbrs_hmm_t *hmm, int sample, int chrom, double *gamma, int32_t *states,
                 int32_t *calls, double *alpha, double *beta, double *delta, double *scaler,
                 double *eprob);

typedef struct gbrs_hmm_info {
    uint64_t total_genes;        /* sum_c n_genes[c]                                        */
    uint64_t algorithmic_bytes;  /* per sample: sum_c n_c * (16 S^2 + 64 S)     */
    /* Device time of the phases of the last run.  For 8 founders (S = 36) the forward, backward and
     * Viterbi chains run concurrently on three streams, so forward (the longer of alpha and
     * delta + backpointers) and backward (sweep + outputs) overlap; last_run_ms is the whole of
     * gbrs_hmm_run on the device. */
    double   last_emission_ms, last_forward_ms, last_backward_ms, last_backtrace_ms;
    int32_t  num_states, n_samples;
    double   last_run_ms;
    /* Blocked scan (1-4 samples): the Viterbi values of the last run by rank convergence - blocks whose values were
     * matched to the block before them, the longest such fix-up in genes, and (sample, chromosome) pairs that were
     * recomputed by the sequential chain because a block did not converge or because a decision of the Viterbi path
     * was closer than the error of the blocks' values (an exact tie, a near-tie).  0 on every other path.
     * last_delta_tie_fallbacks: those of the pairs that were recomputed for a close decision alone (also counted when the
     * blocked scan takes its Viterbi values from max-plus block operators, where the first three stay 0). */
    int32_t  last_delta_blocks, last_delta_longest_fixup, last_delta_fallbacks, last_delta_tie_fallbacks;
} gbrs_hmm_info_t;
int gbrs_hmm_info(gbrs_hmm_t *hmm, gbrs_hmm_info_t *info);

/* Grid pass: `gbrs interpolate` + `gbrs export` on the posteriors the last run left on the device.
 *
 * The knots of one chromosome as `gbrs interpolate` hands them to interp1d (gbrs_utils.py:664-688), host only:
 * [0.0, gene_pos..., grid[n_grid-1] + 1.0] sorted stably (n_genes + 2 knots) and, per knot, the gene whose posterior
 * column it carries (the two end knots repeat the first and the last gene).  A grid point outside the knots fails with
 * scipy's ValueError text, n_genes < 1 with the IndexError the command would raise; both GBRS_ERR_INVALID. */
int gbrs_grid_knots(int n_genes, const double *gene_pos, int n_grid, const double *grid, double *knots,
                    int32_t *knot_gene);

/* The marker grid of the handle; sample independent, it stays on the device like the specificity blocks.
 *   n_grid[c]    grid points of handle chromosome c, 0: the chromosome is not on the grid (grid[c], gene_pos[c] unused)
 *   grid[c]      double[n_grid[c]] positions in file order
 *   n_pos[c]     number of gene positions given: must equal n_genes[c] of the handle
 *   gene_pos[c]  double[n_pos[c]] gene positions in genome order
 * On failure the handle keeps the grid it had. */
int gbrs_hmm_set_grid(gbrs_hmm_t *hmm, const int32_t *n_pos, const double *const *gene_pos, const int32_t *n_grid,
                      const double *const *grid);

/* One device pass over every (sample, chromosome on the grid) of the last run.  sample = -1: all n samples of the run,
 * else that one (n = 1).  M = sum of n_grid[c].  Both outputs are nullable:
 *   dosage      double[n][M][H]   founder dosages (the rows `gbrs export` writes), the chromosomes' grid points in
 *                                 handle order; one device-to-host copy for all samples
 *   gamma_grid  double[n][S * M]  per sample the (S x n_grid[c]) C-order blocks `gbrs interpolate` saves, one after the
 *                                 other in handle order
 * With dosage alone the interpolated states never reach device memory.  GBRS_ERR_STATE before the first run,
 * GBRS_ERR_INVALID without a grid or for a sample out of range; the outputs are untouched on failure. */
int gbrs_hmm_grid(gbrs_hmm_t *hmm, int sample, double *dosage, double *gamma_grid);

/* M of the handle's grid (0 without one) and the device time of the last gbrs_hmm_grid kernel; both nullable. */
int gbrs_hmm_grid_info(gbrs_hmm_t *hmm, int64_t *n_points, double *last_ms);

/* Matching the run's samples against a panel of reference animals (extension; `gbrs reconstruct --match-panel`).
 * With a[s][p][h] the grid dosage of sample s (gbrs_hmm_grid's `dosage`) and b[j][p][h] the dosage of panel entry j on
 * the same grid points, the device forms, for every chromosome c of the handle,
 *   cross[s][c][j]     = sum over the grid points p of c and the founders h of a[s][p][h] * b[j][p][h]
 *   sample_norm[s][c]  = sum of a[s][p][h]^2          panel_norm[j][c] = sum of b[j][p][h]^2
 * and nothing else; a chromosome without grid points gives 0.0 three times.  Every sum is formed by one wavefront in an
 * order that depends on the chromosome alone: a sample's numbers do not depend on the launch it ran in or on whether it
 * was asked for alone, an entry's column not on the entries after it.
 *
 * gbrs_hmm_set_panel: panel[j] is double[M][H] in the layout of `dosage` (grid points of the handle's chromosomes in
 * handle order).  The panel is copied to the device and panel_norm computed there.  Needs a grid (GBRS_ERR_INVALID);
 * a value that is not finite is refused with GBRS_ERR_INVALID naming the entry; n_panel = 0 drops the panel.  On
 * failure the handle keeps the panel it had.  gbrs_hmm_set_grid drops the panel. */
int gbrs_hmm_set_panel(gbrs_hmm_t *hmm, int n_panel, const double *const *panel);

/* sample = -1: all n samples of the run, else that one (n = 1).  cross is double[n][n_chrom][n_panel], sample_norm
 * double[n][n_chrom]; both nullable, one device-to-host copy each.  The dosages are those of the last gbrs_hmm_grid call
 * if it produced dosages for the same `sample` argument since the last run; otherwise the grid kernel runs first, dosage
 * only.  GBRS_ERR_STATE before the first run, GBRS_ERR_INVALID without a panel or for a sample out of range; the outputs
 * are untouched on failure. */
int gbrs_hmm_match(gbrs_hmm_t *hmm, int sample, double *cross, double *sample_norm);

/* Entries of the panel (0 without one), panel_norm double[n_panel][n_chrom], the device time of the last
 * gbrs_hmm_match call's own kernels, and the device memory the panel and the outputs hold; all nullable. */
int gbrs_hmm_match_info(gbrs_hmm_t *hmm, int *n_panel, double *panel_norm, double *last_ms, uint64_t *device_bytes);

/* SNP dosages imputed from the founder haplotypes (extension; `gbrs reconstruct --snp-file`).  A SNP has a chromosome,
 * a position x in the units of the gene positions, and a founder allele pattern m: bit h set when founder h (haplotype
 * order of the handle) carries the alternative allele.  The SNPs of one handle chromosome, in the caller's order, are
 * a grid: their knots and knot_gene are gbrs_grid_knots(n_genes, gene_pos, n_snps_c, snp_pos_c, ...), the end knot the
 * last SNP in that order + 1.0.  With D[i][h] the founder dosage of a sample at gene i (gbrs_genoprob_dosage's loop over
 * the posterior row of gene i), a SNP gives
 *   idx = clip(searchsorted(knots, x, 'left'), 1, n_knots - 1)    g_lo = knot_gene[idx-1], g_hi = knot_gene[idx]
 *   a_lo = 0.0; for h ascending: if bit h of m: a_lo += D[g_lo][h]       a_hi likewise from D[g_hi]
 *   slope = (a_hi - a_lo) / (x_hi - x_lo)      y = slope * (x - x_lo) + a_lo      out = 2.0 * y
 * the expected number of alternative alleles, in [0, 2] up to rounding; no fused multiply-add.  Founders are reduced
 * first and the interpolation comes second; gbrs_hmm_grid interpolates the S states first, so the two differ by
 * reassociation.
 *
 * gbrs_hmm_set_snps: the arguments go per handle chromosome like gbrs_hmm_set_grid's; n_snps[c] = 0: the chromosome has
 * none (its other entries are not read), all zeros drops the SNPs.  Positions, patterns and the int32 knot index of every
 * SNP, found here by one kernel, stay on the device: 16 bytes per SNP.  A pattern with a bit at or above num_haps is
 * GBRS_ERR_INVALID naming chromosome and index; a SNP outside the knots is refused with gbrs_grid_knots' text.  On
 * failure the handle keeps the SNPs it had.  Independent of the handle's grid and panel: neither call disturbs the
 * other. */
int gbrs_hmm_set_snps(gbrs_hmm_t *hmm, const int32_t *n_pos, const double *const *gene_pos, const int32_t *n_snps,
                      const double *const *snp_pos, const uint32_t *const *snp_mask);

/* sample = -1: all n samples of the run, else that one (n = 1).  SNPs first .. first + count in handle order
 * (chromosomes in handle order, the caller's order within); out is double[n][count], one device-to-host copy.  D is made
 * by the first call after a run for a `sample` argument and reused by the calls that follow with the same argument, so
 * a range may be walked in chunks.  count = 0 is accepted and does nothing.  GBRS_ERR_STATE before the first run,
 * GBRS_ERR_INVALID without SNPs, for a range outside 0 .. M or a sample out of range; out is untouched on failure. */
int gbrs_hmm_impute(gbrs_hmm_t *hmm, int sample, int64_t first, int64_t count, double *out);

/* M of the handle's SNPs (0 without any), the device time of the last gbrs_hmm_impute call's kernels (0.0 until a pass
 * has run on the handle), and the device memory the SNPs, D and the output chunk hold; all nullable. */
int gbrs_hmm_impute_info(gbrs_hmm_t *hmm, int64_t *n_snps, double *last_ms, uint64_t *device_bytes);

/* The parts of those times, in device milliseconds: the search kernel of the last gbrs_hmm_set_snps, and of the last
 * gbrs_hmm_impute call the kernel that made D (0.0 when D was reused) and the imputation kernel; all nullable. */
int gbrs_hmm_impute_times(gbrs_hmm_t *hmm, double *setup_ms, double *dosage_ms, double *kernel_ms);

/* Diplotype paths drawn from the joint posterior of the last run (extension; forward-filter / backward-sample on the
 * run's filtered forward values, which the first call makes like gbrs_hmm_get(alpha)).  sample = -1: all n samples of
 * the run, else that one (n = 1).  Draw d of a sample, chromosome c, genes i = n_c - 1 .. 0:
 *   l_k = alpha[k][i] (+ T[i][z_{i+1}][k] below the last gene), w_k = exp(l_k), c_k = w_0 + .. + w_k, t = u * c_{S-1};
 *   z_i = the smallest k with c_k > t; none by rounding: the largest k with w_k > 0; c_{S-1} zero or not finite: the first
 *   argmax of l_k, counted in `degenerate`.
 *   u = ((a >> 5) * 2^26 + (b >> 6)) * 2^-53 with a, b the words 2 (i & 1) and 2 (i & 1) + 1 of Philox4x32-10 on the
 *   counter (i >> 1, c, d, stream) and the key (seed lo, seed hi).
 *   streams     uint32[n] ids of the samples of this call; NULL: the sample's index in the run.  A sample's draws are a
 *               function of (seed, its stream, c, d, i) and of its run alone: not of its slot, the batch or the slabs.
 *   paths       uint8[n][n_draws][total_genes] state indices, a draw's chromosomes one after the other in handle order
 *   changes     int32[n][n_draws][n_chrom], nullable: founder changes along the draw, 2 - |{a,b} n {c,d}| (multisets)
 *               summed over neighbouring genes
 *   degenerate  nullable: decisions of this call that fell back to the argmax
 * Large requests go through the device in slabs of draws (about 1 GiB of device memory).  GBRS_ERR_STATE before the
 * first run; GBRS_ERR_INVALID for n_draws < 1, a sample out of range or paths == NULL; outputs untouched on failure. */
int gbrs_hmm_sample_paths(gbrs_hmm_t *hmm, int sample, int n_draws, uint64_t seed, const uint32_t *streams, uint8_t *paths,
                          int32_t *changes, uint64_t *degenerate);

/* Device time of the last gbrs_hmm_sample_paths call's kernels (all slabs) and the device memory its buffers hold; both
 * nullable. */
int gbrs_hmm_sample_info(gbrs_hmm_t *hmm, double *last_ms, uint64_t *device_bytes);

/* Diagnostics of the last run (extension; R/qtl2's count_xo / locate_xo without the draws, and calc_errorlod per gene).
 * sample = -1: all n samples of the run, else that one (n = 1).  Every output is [n][total_genes], a sample's chromosomes
 * one after the other in handle order, and nullable; a pass none of whose outputs is asked for is not launched.
 * With k the state at gene i and j the state at gene i + 1 of a chromosome, E the log emission rows, iv the prior:
 *   lx[k][j]  = alpha[k][i] + T[i][j][k] + E[i+1][j] + beta[j][i+1],  x = exp(lx - max lx)  (0 where lx is -inf)
 *   xo        [i]: sum x * change[k][j] / sum x, the expected founder changes (2 - |{a,b} n {c,d}|, multisets) between
 *             genes i and i + 1; the slot of a chromosome's last gene is 0.0
 *   pswitch   [i]: sum over k != j of x / sum x, the probability that the diplotype changes; last gene's slot 0.0
 *   errlod    [i]: (lse(iv + E[i]) - (lse(alpha[:,i] + beta[:,i]) - lse((alpha[:,i] - E[i]) + beta[:,i]))) / ln 10 with
 *             lse(v) = max v + log sum exp(v - max v), an entry whose alpha is -inf carrying weight 0: log10 of how much
 *             better the prior predicts gene i's data than the chromosome's other genes do
 *   maxmarg   [i]: the first index of the largest gamma[:, i];  maxprob [i]: that value
 * Only T[0 .. n_c - 2] of a chromosome are read.  GBRS_ERR_STATE before the first run, GBRS_ERR_INVALID for a sample out
 * of range: both before any launch, the outputs untouched. */
int gbrs_hmm_diagnostics(gbrs_hmm_t *hmm, int sample, double *xo, double *pswitch, double *errlod, double *maxprob,
                         int32_t *maxmarg);

/* The pair posteriors of one (sample, chromosome) of the last run: xi[i][k][j] = x[k][j] / sum x of the interval
 * i -> i + 1 as above, double[n_c - 1][S][S]; nothing is written for a chromosome of one gene.  GBRS_ERR_STATE before the
 * first run; GBRS_ERR_INVALID for a sample or chromosome out of range or xi == NULL; xi untouched on failure. */
int gbrs_hmm_pair_posterior(gbrs_hmm_t *hmm, int sample, int chrom, double *xi);

/* Device time of the last gbrs_hmm_diagnostics call's kernels (0 if none ran); nullable. */
int gbrs_hmm_diagnostics_info(gbrs_hmm_t *hmm, double *last_ms);

/* Data log-likelihood of the last run under the handle's own tables (extension): per (sample,
 * chromosome) the sum over the chromosome's genes of log Z_i, Z_i the normaliser of gene i in the scaled forward recursion,
 * i.e. minus the sum of the `scaler` row gbrs_hmm_get returns.  One reduction over what the forward pass kept; the order
 * of the sum depends on the chromosome's length alone, so a value is the same bits in every batch and slot.
 * sample = -1: all n samples of the run, else that one (n = 1).  loglik is double[n][n_chrom].  GBRS_ERR_STATE before the
 * first run; GBRS_ERR_INVALID for a sample out of range or loglik == NULL; both before any launch, loglik untouched. */
int gbrs_hmm_loglik(gbrs_hmm_t *hmm, int sample, double *loglik);

/* Data log-likelihood of the last run's emissions on chromosome `chrom` under n_tables other transition tables: table k
 * is double[n_trans[k]][S][S] in natural log, T[i][to][from] as for gbrs_hmm_create (-inf entries are legal); only
 * T[0 .. n_c - 2] are read, none for a chromosome of one gene (tprob[k] may then be NULL).  One launch runs the forward
 * recursion alone for every (table, sample) pair:
 *   gene 0: y_j = exp(init_j) * pe_0[j];  gene i: x_j = (sum_k y_{i-1}[k] * exp(T[i-1][j][k])) / Z_{i-1} + tiny,
 *   y_j = x_j * pe_i[j], Z_i = sum_j y_j;  result = sum_i log Z_i added in gene order, -inf if a Z_i is 0 or not finite.
 * loglik is double[n_tables][n] (sample = -1: n = all samples of the run, else 1).  The handle's tables and the run's
 * results are not touched.  Device memory: n_tables x (n_c - 1) x S^2 x 16 bytes, kept for later calls.
 * GBRS_ERR_STATE before the first run; GBRS_ERR_INVALID for a sample or chromosome out of range, n_tables < 1, an
 * n_trans[k] < n_c - 1, or a NULL n_trans, tprob, needed tprob[k] or loglik; all before any launch, loglik untouched. */
int gbrs_hmm_loglik_tables(gbrs_hmm_t *hmm, int chrom, int n_tables, const int32_t *n_trans, const double *const *tprob,
                           int sample, double *loglik);

/* Device time of the last gbrs_hmm_loglik / gbrs_hmm_loglik_tables call's kernels (0 if none ran) and the device memory
 * the two calls' buffers hold; both nullable. */
int gbrs_hmm_loglik_info(gbrs_hmm_t *hmm, double *last_ms, uint64_t *device_bytes);

int gbrs_hmm_destroy(gbrs_hmm_t *hmm);

/* `gbrs interpolate` numeric body (gbrs/gbrs_utils.py:684-688): the rows of y (S x n_points, C
 * order) given at ascending positions x are linearly interpolated onto x_grid with scipy
 * interp1d(kind='linear')'s operation order; out is (S x n_grid).  The caller pads the gene
 * positions / posterior columns with the reference's two end points (:664-676, :684-685).  Grid
 * points outside [x[0], x[n_points-1]] fail with scipy's ValueError text. */
int gbrs_interpolate(int num_states, int n_points, const double *x, const double *y,
                     int n_grid, const double *x_grid, double *out, int device);

/* `gbrs export` numeric body (gbrs_utils.py:888-927): n_rows x S diplotype probabilities times the
 * (S x H) matrix 0.5 * (founder count in diplotype) -> n_rows x H founder dosages. */
int gbrs_genoprob_dosage(int num_haps, int64_t n_rows, const double *gprob, double *out, int device);

/* `gbrs get-transition-prob` numeric body for the `RI` mating scheme (gbrs/gbrs_utils.py:101-187 ris_step, forward
 * direction; :269-290): the log transition tables of two-founder recombinant inbred lines by sib mating, all
 * chromosomes in one launch.  cm holds the markers' cM positions, chromosome c's at [chrom_ptr[c], chrom_ptr[c+1]) in
 * file order; is_x[c] != 0 selects the X-chromosome formulas.  A chromosome of n_c markers has max(n_c - 1, 0)
 * intervals d = cm[m+1] - cm[m], every d < epsilon (zero and negative steps too) replaced by epsilon, and no interval
 * reaches across a chromosome boundary.  out receives 9 doubles per interval, the chromosomes one after the other: the
 * (3 x 3) natural-log table in the reference's element order ([dt1][dt2] = ris_step(gen_left = dt1, gen_right = dt2)
 * over AA, AB, BB), each entry log(a) - log(1 + gamma) as two logarithms and a subtraction.  chrom_ptr must start at 0 and not decrease (GBRS_ERR_INVALID); no
 * interval at all is a success without a launch (out may then be NULL). */
int gbrs_ri_transition_tables(const double *cm, const int64_t *chrom_ptr /* num_chroms + 1 */,
                              const uint8_t *is_x /* num_chroms */, int64_t num_chroms, double gamma_scale,
                              double epsilon, int device, double *out /* 9 * sum_c max(n_c - 1, 0) */);

/* `gbrs get-alignment-spec` numeric body (gbrs/gbrs_utils.py:335-372): tables is [F][num_genes][num_strains], one
 * (genes x strains) TPM table per report file that exists, the files of strain i at [strain_ptr[i], strain_ptr[i+1]);
 * strain_div[i] is the number of files the strain lists (missing ones included, >= its tables).  Per strain the tables
 * are added in file order starting from 0 and divided once by strain_div[i]: row i of axes[g] (G x S x S).  ases[g][i]
 * (G x S) is that row summed left to right; avecs[g] row i is the row divided by its Euclidean norm when its sum exceeds
 * 1e-6, else the row itself; has_avec[g] = 1 when some ases[g][i] > min_expr (the reference writes avecs[g] only then).
 * axes and ases are bit-identical to numpy's; avecs differs by the rounding of the norm.  num_strains outside 1..32 is
 * GBRS_ERR_UNSUPPORTED; num_genes == 0 is a success without a launch. */
int gbrs_alignment_spec(const double *tables, const int64_t *strain_ptr /* num_strains + 1 */,
                        const int64_t *strain_div /* num_strains */, int64_t num_genes, int num_strains, double min_expr,
                        int device, double *axes, double *ases, double *avecs, uint8_t *has_avec);

/* ------------------------------------------------------------------------------------------
 * Genome scan (extension; `gbrs reconstruct --scan-pheno`, `gbrs scan`): Haley-Knott regression of
 * phenotypes on the founder dosages of a cohort at every grid point, with additive covariates.
 * ---------------------------------------------------------------------------------------- */

typedef struct gbrs_scan gbrs_scan_t;

/* The handle of one cohort on one grid: n_chrom chromosomes of points_per_chrom[c] >= 0 grid points (M their sum, in
 * that order, as gbrs_hmm_grid lays them out) and num_haps founders.  num_haps < 2 or > 17, n_chrom < 1 and M = 0 are
 * GBRS_ERR_INVALID.  The handle is independent of any HMM handle. */
int gbrs_scan_create(int device, int n_chrom, const int32_t *points_per_chrom, int num_haps, gbrs_scan_t **out);
int gbrs_scan_destroy(gbrs_scan_t *scan);

/* n more samples at the end of the cohort: dosage is double[n][M][H] on the host (gbrs_hmm_grid's `dosage`).  A value
 * that is not finite is refused with GBRS_ERR_INVALID naming the entry; the cohort is then as it was.  An append drops
 * what gbrs_scan_prepare made. */
int gbrs_scan_append(gbrs_scan_t *scan, int n, const double *dosage);

/* The same from the grid dosages an HMM handle holds for its last run, device to device: sample = -1 appends all samples
 * of the run in their order, else that one.  The grid kernel runs first under gbrs_hmm_match's condition (the handle
 * holds no dosages of the last run for the same `sample` argument), and only after every check below has passed: a
 * refused call launches nothing on the HMM handle.  GBRS_ERR_STATE before the first run;
 * GBRS_ERR_INVALID without a grid, for a sample out of range, for another device, and for a handle whose grid has other
 * points per chromosome or whose founder count differs.  What the cohort holds afterwards is, bit for bit, what
 * gbrs_scan_append of gbrs_hmm_grid's output would have left. */
int gbrs_scan_append_hmm(gbrs_scan_t *scan, gbrs_hmm_t *hmm, int sample);

/* The phenotype-independent part, once per (cohort, covariates).  qz is double[n][c]: an orthonormal basis of the
 * covariates' columns (the caller's QR; its span holds the intercept).  Per grid point m, with X_m = D[:, m, 0:H-1]:
 *   X~ = X_m - qz qz' X_m,  G = X~' X~,
 *   Cholesky of G in column order j = 0 .. H-2 with the skip rule: the pivot is d_j = G_jj - sum over the kept i < j of
 *   L_ji^2; column j is kept iff G_jj > 0 and d_j > 1e-10 G_jj; a skipped column has a zero row in L and takes no part
 *   in anything after it.  The covariates count as the columns before column 0: G_jj <= 1e-10 |X_m[:, j]|^2 (the
 *   projection left rounding: a founder with the same dosage in every sample) is taken as G_jj = 0,
 *   W_m = L^-1 X~' (zero rows for skipped columns), rank[m] = number of kept columns.
 * W is kept on the device as [M * Hp][n_ld], Hp = 8 for H <= 9 and 16 otherwise, n_ld = n rounded up to 32 and zero
 * filled.  GBRS_ERR_INVALID for c < 1 or c > 64, n <= c + H - 1, and a qz value that is not finite (the message names
 * the entry); such a refusal leaves the handle as it was, an earlier preparation included.  A failure after these
 * checks (device memory, the kernel) leaves it unprepared. */
int gbrs_scan_prepare(gbrs_scan_t *scan, int c, const double *qz);

/* P phenotypes of the prepared cohort: pheno is double[n][P], rows in append order.  Per phenotype p
 *   y~ = y - qz qz' y,  rss0 = |y~|^2,  ess[m] = |W_m y~|^2,  rss1 = rss0 - ess[m],
 *   lod[p][m] = (n / 2) log10(rss0 / rss1); 0.0 where rss0 == 0; +inf where rss1 <= 0 < rss0.
 * lod is double[P][M] (nullable), peak_lod double[P][n_chrom] the maximum over a chromosome's points, peak_index
 * int64[P][n_chrom] its grid index among the M points, the lowest on ties (NaN and -1 for a chromosome without points);
 * both nullable.  The phenotypes go through the device in chunks of 512 columns; the products W_m y~ never reach memory.
 * A phenotype's numbers are the same bits alone or among others, at any column, in any chunk, and however the cohort
 * was appended.  Nothing here looks for a phenotype that lies in the covariates' span: a column whose values are all
 * equal projects to rounding, not to zeros, unless the projection happens to be exact, and its LODs are then noise; the
 * caller sends such a column as zeros (gbrs_amd.scan.GenomeScan.run does), which gives rss0 == 0 and 0.0 throughout.
 * GBRS_ERR_INVALID before gbrs_scan_prepare, for P < 1 and for a value that is not finite (the message
 * names the entry); the outputs are untouched on failure. */
int gbrs_scan_run(gbrs_scan_t *scan, int64_t P, const double *pheno, double *lod, double *peak_lod, int64_t *peak_index);

typedef struct gbrs_scan_info {
    int64_t  n, M;               /* samples appended, grid points                                              */
    int32_t  H, c;               /* founders; covariate columns of the last prepare (0: not prepared)          */
    double   last_prepare_ms;    /* device time of the last gbrs_scan_prepare's kernel                         */
    double   last_run_ms;        /* device time of the last gbrs_scan_run: its kernels and copies, all chunks  */
    double   last_product_ms;    /* of that, the product kernel alone, summed over the chunks                  */
    uint64_t device_bytes;       /* what the handle holds on the device                                        */
} gbrs_scan_info_t;
/* rank is int32[M] of the last prepare, nullable; untouched when the handle is not prepared. */
int gbrs_scan_info(gbrs_scan_t *scan, gbrs_scan_info_t *info, int32_t *rank);

/* Permutation thresholds of the scan: perm_max[p][b], the largest LOD phenotype p reaches anywhere on the
 * selected chromosomes under permutation b = 0 .. B-1.  Freedman-Lane: the residuals of the reduced model are permuted,
 * not the dosage rows, so W of gbrs_scan_prepare serves every permutation.  Per (p, b):
 *   y~ = y - qz qz' y, as gbrs_scan_run forms it (the same kernel);
 *   key of sample s: k_s = (w0 << 32) | w1, the words 0 and 1 of Philox4x32-10 on the counter
 *   (s & 0xFFFFFFFF, s >> 32, b & 0xFFFFFFFF, b >> 32) with the key (seed & 0xFFFFFFFF, seed >> 32);
 *   perm_b(s) = the rank of (k_s, s) among the n pairs in lexicographic order: it depends on (seed, b, n) alone and is the
 *   same for every phenotype;
 *   y*[s] = y~[perm_b(s)],  y*~ = y* - qz qz' y*,  rss0* = |y*~|^2,  ess*[m] = |W_m y*~|^2, and the LOD by gbrs_scan_run's
 *   formula with its two edge rules;
 *   perm_max[p][b] = the maximum over the grid points of the chromosomes c with chrom_mask[c] != 0 (NULL: all).
 * pheno is double[n][P] as for gbrs_scan_run (a constant column goes in as zeros and gives 0.0 throughout), perm_max
 * double[P][B], perm_index int32[B][n] the permutations themselves (nullable).  Nothing per permutation is uploaded and
 * no LOD leaves the device: the columns p B + b pass through the product kernel in gbrs_scan_run's chunks of 512, and
 * the device holds y~ [P][n_ld], the permutations [B][n], perm_max and one chunk's buffers next to what the handle
 * holds.  The ranks are found by counting, n^2 comparisons per permutation.  perm_max[p][b] is the same bits for any P,
 * B > b, column and chunk, and however the cohort was appended.  GBRS_ERR_INVALID before gbrs_scan_prepare, for P < 1,
 * for B < 1, for a mask that selects no grid point and for a phenotype value that is not finite (the message names the
 * entry); the outputs are untouched on failure.  The call allocates and frees its own buffers: what the handle holds,
 * gbrs_scan_run's bits and gbrs_scan_info_t are as before. */
int gbrs_scan_permute(gbrs_scan_t *scan, int64_t P, const double *pheno, int64_t B, uint64_t seed,
                      const uint8_t *chrom_mask /* [n_chrom], nullable */, double *perm_max, int32_t *perm_index);

typedef struct gbrs_scan_perm_info {
    int64_t  P, B;               /* of the last gbrs_scan_permute (0: none yet)                                  */
    double   last_permute_ms;    /* device time of the pass: uploads, projections, ranks, all chunks            */
    double   last_product_ms;    /* of that, the product kernel alone, summed over the chunks                   */
    uint64_t peak_device_bytes;  /* what the handle held during the pass, the call's own buffers included       */
} gbrs_scan_perm_info_t;
int gbrs_scan_perm_info(gbrs_scan_t *scan, gbrs_scan_perm_info_t *info);

/* SNP association on the scan handle: every founder SNP is tested with one degree of freedom on the allele
 * dosage that its founder pattern implies, from the cohort's grid dosages where they lie.  No fused multiply-add anywhere.
 *
 * Where a SNP lies.  A SNP has a chromosome c of the handle, a position x in the units of the grid positions and a founder
 * pattern m: bit h of m is set when founder h carries the alternative allele.  With g[0..k-1] the grid positions of
 * chromosome c in the handle's point order:
 *   lo = clip(searchsorted(g, x, 'right') - 1, 0, k-1),  hi = min(lo + 1, k-1),
 *   t = (x - g[lo]) / (g[hi] - g[lo]) if g[hi] > g[lo] and x > g[lo], else 0.0;  then t = min(t, 1.0).
 * A SNP outside the grid takes the end point's dosage, as np.interp does; a SNP on a duplicated grid position takes the
 * last of the equal points.
 * Its dosage for sample s:  a_lo = 0.0; for h ascending: if bit h of m: a_lo += D[s][lo][h];  a_hi likewise from D[s][hi];
 *   x_s = 2.0 * (a_lo + t * (a_hi - a_lo)).
 *
 * gbrs_scan_set_snps: the arguments go per chromosome, as gbrs_hmm_set_snps takes them: grid_pos[c] is double[points of c]
 * (nullable for a chromosome without points), n_snps[c] >= 0, snp_pos[c] double[n_snps[c]], snp_mask[c] uint32[n_snps[c]].
 * The SNPs are numbered in handle order: chromosome after chromosome, each in the order given (sorted by position they
 * share grid intervals, which the pass makes use of; any order is valid and gives the same bits per SNP).  The host checks
 * everything first: GBRS_ERR_INVALID for a grid or SNP position that is not finite, grid positions that decrease (naming
 * chromosome and index), a pattern bit at or above H (naming chromosome and index) and a SNP on a chromosome without grid
 * points.  Positions and patterns are uploaded and one kernel finds lo (the global point index), hi and t per SNP; 20 bytes
 * per SNP stay on the device (lo, hi, pattern: 4 each; t: 8).  All-zero counts drop the SNPs.  On failure the handle
 * keeps what it had.  The call is independent of gbrs_scan_prepare, and appending samples does not drop the SNPs. */
int gbrs_scan_set_snps(gbrs_scan_t *scan, const double *const *grid_pos, const int64_t *n_snps,
                       const double *const *snp_pos, const uint32_t *const *snp_mask);

/* x_s of the SNPs first .. first + count - 1 for every sample: out is double[n][count].  Needs SNPs and a cohort, not a
 * preparation; GBRS_ERR_INVALID without either and for a range outside the handle's SNPs. */
int gbrs_scan_snp_dosage(gbrs_scan_t *scan, int64_t first, int64_t count, double *out);

/* The test of every SNP on the prepared cohort (qz, c of gbrs_scan_prepare).  Every sum over the samples is one
 * wavefront's, in gbrs_scan_prepare's order: lane l adds the samples l, l + 64, ... in order, and the 64 partial sums meet
 * in a butterfly.
 *   raw = sum x_s^2,  qtx[k] = sum_s qz[s][k] x_s,
 *   x~_s = x_s - sum_k (k ascending) qz[s][k] qtx[k],  G = sum x~_s^2;
 *   the SNP is used iff G > 0 and G > 1e-10 raw (gbrs_scan_prepare's threshold with its meaning: a SNP that is monomorphic
 *   in the cohort, the all-zeros and the all-ones pattern project to rounding and are not tested);
 *   w = x~ / sqrt(G), a true division; zeros for an unused SNP;
 *   per phenotype p, y~ and rss0 as gbrs_scan_run forms them (the same kernel): ess = (w . y~_p)^2 and the LOD by
 *   gbrs_scan_run's formula with its two edge rules; an unused SNP has LOD 0.0 for every phenotype.
 * pheno is double[n][P] as for gbrs_scan_run.  lod is double[P][M_snp], used uint8[M_snp], peak_lod double[P][n_chrom] the
 * largest LOD over the used SNPs of a chromosome, peak_index int64[P][n_chrom] that SNP's index in handle order, the
 * lowest on ties (NaN and -1 for a chromosome without a used SNP); all four nullable.  SNP chunks (gbrs_scan_snp_info's
 * `chunk`) are the outer loop and phenotype chunks of 512 the inner one: a SNP's row w is built once per call, y~ of all P
 * stays on the device as [P][n_ld], and neither the dosage matrix [n][M_snp] nor the products reach memory beyond one
 * chunk's rows.  A SNP's LODs are the same bits alone or among others, at any place in its 64-row tile, in any chunk, for
 * any P, column and phenotype chunk, and however the cohort was appended.  GBRS_ERR_INVALID before gbrs_scan_prepare,
 * without SNPs, for P < 1 and for a value that is not finite (the message names the entry); the outputs are untouched on
 * such a failure.  The call allocates and frees its own buffers: the handle's W, gbrs_scan_run's bits and
 * gbrs_scan_info_t are as before.  The allele effect, permutations of the SNP scan and SNP x covariate interactions are
 * not computed. */
int gbrs_scan_snps(gbrs_scan_t *scan, int64_t P, const double *pheno, double *lod, uint8_t *used, double *peak_lod,
                   int64_t *peak_index);

typedef struct gbrs_scan_snp_info {
    int64_t  M_snp;              /* SNPs on the handle                                                           */
    int64_t  chunk;              /* SNPs whose rows are on the device at a time in gbrs_scan_snps                */
    int64_t  P;                  /* of the last gbrs_scan_snps (0: none yet)                                     */
    double   last_pass_ms;       /* device time of the last pass: uploads, projections, all chunks, copies       */
    double   last_row_ms;        /* of that, the row kernel, summed over the SNP chunks                          */
    double   last_product_ms;    /* of that, the product kernel, summed over the chunks                          */
    uint64_t device_bytes;       /* what the SNPs hold on the device (not part of gbrs_scan_info_t's figure)     */
    uint64_t peak_device_bytes;  /* what the handle held during the last pass, the call's own buffers included   */
    int32_t  staged;             /* the last pass's row kernel: 1 the two grid points of a run of SNPs in LDS, 0 (they  */
    int32_t  reserved;           /* do not fit a workgroup's share) every SNP read the cohort itself; the same bits     */
} gbrs_scan_snp_info_t;
int gbrs_scan_snp_info(gbrs_scan_t *scan, gbrs_scan_snp_info_t *info);

/* Mediation of QTL peaks on the scan handle: for target t - a phenotype column y_t and a grid point
 * m = point[t] in [0, M) - every mediator column z_q joins the covariates in turn and the LOD of y_t at m is formed again.
 * A mediator whose inclusion makes the LOD collapse is a candidate for what lies between the locus and the target.  W_m of
 * gbrs_scan_prepare serves every pair: no new factorisation.  No fused multiply-add anywhere.
 *   y~_t, z~_q = v - qz qz' v as gbrs_scan_run forms y~ (the same kernel); a constant column goes in as zeros
 *   s_yy = |y~_t|^2        s_zz = |z~_q|^2        s_yz = y~_t . z~_q
 *   a = W_m y~_t           b = W_m z~_q
 *   rss1 = s_yy - |a|^2                           lod0[t] = (n/2) log10(s_yy / rss1), gbrs_scan_run's formula and edge rules
 *   e_zz = s_zz - |b|^2    e_yz = s_yz - a . b
 *   rss0' = s_yy - s_yz^2 / s_zz                  (the target given covariates + mediator)
 *   rss1' = rss1 - e_yz^2 / e_zz                  (given covariates + mediator + founders at m)
 *   lod_med[t][q] = (n/2) log10(rss0' / rss1'), 0.0 where rss0' == 0, +inf where rss1' <= 0 < rss0'
 * used[t][q] = 0 and lod_med[t][q] = NaN when s_zz == 0 (the mediator lies in the covariates' span), when
 * e_zz <= 1e-10 s_zz (it lies in the span of covariates + founders at m: gbrs_scan_prepare's threshold) or when
 * rss0' <= 1e-10 s_yy (the target lies in the span of covariates + mediator, as for q = the target itself).
 * Per target over its used mediators only: n_used[t]; mean[t] and sd[t] of lod_med (two passes, n_used - 1 in the
 * denominator, NaN below 2 used mediators; the order of the sums depends on Q alone); best_index[t][k], best_lod[t][k] for
 * k < K <= 64: the K used mediators with the lowest lod_med in ascending (lod_med, mediator index) order, -1 / NaN in the
 * places past n_used.
 * target is double[n][T], point int64[T], mediator double[n][Q]; lod0 double[T], lod_med double[T][Q], used uint8[T][Q],
 * best_lod double[T][K], best_index int64[T][K], mean, sd double[T], n_used int64[T]; lod0, lod_med, used, mean, sd and
 * n_used are nullable, best_* with K = 0.  The projected mediators stay on the device as [Q][n_ld]; the targets pass in
 * chunks of 512, whose [512][Q] LODs live on the device only unless lod_med / used ask for them, so device memory is
 * bounded for any T.  The sums over the samples of a and of the projections are one wavefront's in gbrs_scan_prepare's
 * order; b, a . b and s_yz come from one f64 MFMA product of the gathered W rows with the mediators, each a fixed chain.
 * The numbers of a pair are the same bits alone or among others, at any target and mediator position, in any chunk, for
 * any K and however the cohort was appended.  GBRS_ERR_INVALID before gbrs_scan_prepare, for T < 1, Q < 1, K < 0 or
 * K > 64, a point outside [0, M), n <= c + H (the mediator takes one more degree of freedom than the scan) and a value
 * that is not finite (the message names the entry); the outputs are untouched on such a failure.  The call allocates and
 * frees its own buffers: what the handle holds, gbrs_scan_run's bits and gbrs_scan_info_t are as before.  No mixed model,
 * no more than one mediator at a time, no mediation at SNPs. */
int gbrs_scan_mediate(gbrs_scan_t *scan, int64_t T, const double *target, const int64_t *point, int64_t Q,
                      const double *mediator, int K, double *lod0, double *lod_med, uint8_t *used, double *best_lod,
                      int64_t *best_index, double *mean, double *sd, int64_t *n_used);

typedef struct gbrs_scan_mediate_info {
    int64_t  T, Q;               /* of the last gbrs_scan_mediate (0: none yet)                                  */
    double   last_pass_ms;       /* device time of the pass: uploads, projections, all chunks, copies            */
    double   last_product_ms;    /* of that, the product kernel alone, summed over the target chunks             */
    uint64_t peak_device_bytes;  /* what the handle held during the pass, the call's own buffers included        */
} gbrs_scan_mediate_info_t;
int gbrs_scan_mediate_info(gbrs_scan_t *scan, gbrs_scan_mediate_info_t *info);

/* Founder effects at QTL peaks on the scan handle (R/qtl2's scan1coef at chosen points): for target t - the
 * phenotype column y = column[t] in [0, P) and the grid point m = point[t] in [0, M) - the effects of all H founders and
 * their standard errors.  W_m of gbrs_scan_prepare serves, as it does for mediation: no new factorisation of the design.
 * No fused multiply-add anywhere.
 *   y~, rss0 as gbrs_scan_run forms them (the same kernel); a constant column goes in as zeros
 *   S = the kept rows of W_m,  r = rank[m],  a = W_S y~
 *   X~_j, j < H-1: founder j's dosage column at m with the covariates projected out, by gbrs_scan_prepare's steps and in
 *   their order;  X~_{H-1} = -sum_{j<H-1} X~_j (j ascending) by definition: the sum constraint the scan assumes when it
 *   drops founder H-1, which keeps the rule well defined for dosage rows that do not add up to a constant
 *   R = W_S [X~_0 .. X~_{H-1}] (r x H; its last column is minus the sum of the others, in the same order),  C = R R',
 *   symmetric positive definite because R has full row rank: a plain Cholesky without a skip rule
 *   effect = R' C^-1 a: the minimum-norm least-squares solution over all H founder columns, pinv([X~_0 .. X~_{H-1}]) y~.
 *   At full rank the effects add up to zero (qtl2's zero-sum founder effects); a founder j < H-1 without dosage in the
 *   cohort at m gets exactly 0.0 with se 0.0; founders with identical dosages share their effect equally; with r = 0
 *   every effect and se is 0.0
 *   rss1 = max(rss0 - |a|^2, 0),  sigma2 = rss1 / (n - c - r) (the divisor is positive under gbrs_scan_prepare's check),
 *   se[h] = sqrt(sigma2) |C^-1 R[:, h]|
 *   lod[t] by gbrs_scan_run's formula with its two edge rules on this pass's rss0 and |a|^2.  It lies within rounding of
 *   gbrs_scan_run's value at (y, m) and does not carry its bits: that one is an MFMA chain, this one a wavefront sum.
 * pheno is double[n][P] as for gbrs_scan_run; effect and se double[T][H], lod and sigma2 double[T], rank int32[T] (rank[m]
 * of gbrs_scan_info); every output nullable.  y~ of all P columns stays on the device as [P][n_ld]; the targets pass in
 * chunks of 512, one workgroup each, so device memory is bounded for any T.  Every sum over the samples is one
 * wavefront's in gbrs_scan_prepare's order and the small dense steps run in a fixed order, without atomics: a target's
 * numbers are the same bits alone or among others, at any place in the list, in any chunk, for any P and any position of
 * its column, given twice, and however the cohort was appended.  GBRS_ERR_INVALID before gbrs_scan_prepare, for P < 1 or
 * T < 1, for a column outside [0, P) or a point outside [0, M) and for a value that is not finite (the message names the
 * entry); the outputs are untouched on such a failure.  The call allocates and frees its own buffers: what the handle
 * holds, gbrs_scan_run's bits and gbrs_scan_info_t are as before.  No mixed model, no BLUP shrinkage of the effects, no
 * Bayes credible interval. */
int gbrs_scan_effects(gbrs_scan_t *scan, int64_t P, const double *pheno /* [n][P] */, int64_t T,
                      const int64_t *column /* [T], in [0,P) */, const int64_t *point /* [T], in [0,M) */,
                      double *effect /* [T][H] */, double *se /* [T][H] */, double *lod /* [T] */,
                      double *sigma2 /* [T] */, int32_t *rank /* [T] */);

typedef struct gbrs_scan_effects_info {
    int64_t  T, P;               /* of the last gbrs_scan_effects (0: none yet)                                  */
    double   last_pass_ms;       /* device time of the pass: uploads, projections, all chunks, copies            */
    uint64_t peak_device_bytes;  /* what the handle held during the pass, the call's own buffers included        */
} gbrs_scan_effects_info_t;
int gbrs_scan_effects_info(gbrs_scan_t *scan, gbrs_scan_effects_info_t *info);

/* gbrs_scan_run with LOD support intervals (R/qtl2's lod_int): the pass of gbrs_scan_run - the same kernels,
 * the same bits in lod, peak_lod and peak_index - and one more kernel after the peaks on each chunk's LOD rows while they
 * are on the device.  For phenotype p on a chromosome with peak index k and peak value v:
 *   support_lo = the largest index i < k of the chromosome with lod[i] <= v - drop, its first point if there is none;
 *   support_hi = the smallest index i > k with lod[i] <= v - drop, its last point if there is none.
 * Both are grid indices among the M points - the flanking points where the LOD has fallen - int64[P][n_chrom], nullable,
 * and -1 for a chromosome without points.  There is no arithmetic beyond the one subtraction.  GBRS_ERR_INVALID for a
 * drop that is negative or not finite; the other refusals are gbrs_scan_run's, and the outputs are untouched on failure.
 * The two tables of a chunk are the call's own: gbrs_scan_info_t's device_bytes is what gbrs_scan_run leaves. */
int gbrs_scan_run_support(gbrs_scan_t *scan, int64_t P, const double *pheno, double drop, double *lod, double *peak_lod,
                          int64_t *peak_index, int64_t *support_lo, int64_t *support_hi /* [P][n_chrom] */);

/* Linear mixed model with leave-one-chromosome-out kinship on the scan handle (R/qtl2's scan1 with
 * kinship = calc_kinship(probs, "loco")): the phenotype has a polygenic random effect whose covariance is the kinship of
 * the chromosomes other than the scanned one, y ~ N(Z b + X_m a, s2 (h K + (1 - h) I)).  No fused multiply-add anywhere.
 *
 * Kinship.  With A_c the cohort's dosages on chromosome c as [n][M_c H] and S_c = A_c A_c',
 *   K = scale * (sum over the chromosomes c != leave_out of S_c, added in chromosome order) / (sum of their M_c);
 * leave_out = -1 leaves none out (the overall kinship).  K is double[n][n] and symmetric bit for bit.  S_c is an f64 MFMA
 * product, one chain per entry over the columns in order, without atomics; all S_c are formed at the first call and stay
 * on the device until the next append.  The LODs below do not depend on scale, the heritabilities do; gbrs_amd passes
 * 2 / t^2 with t the total of a point's dosages (qtl2's doubled kinship of allele probabilities).  GBRS_ERR_INVALID for a
 * cohort without samples or of more than 4096, for a leave_out outside -1 .. n_chrom-1, for a scale that is not finite
 * and for a chromosome whose complement has no grid points; K is untouched on failure. */
int gbrs_scan_kinship(gbrs_scan_t *scan, int leave_out /* -1: none */, double scale, double *K /* [n][n] */);

/* The phenotype-independent part of the mixed model, once per (cohort, covariates, kinships).  The caller factors each
 * distinct kinship K_e = U_e diag(lambda_e) U_e' (gbrs_amd: numpy.linalg.eigh) and passes n_eig pairs - U[e] double[n][n]
 * with the eigenvectors in its columns, lambda[e] double[n] - and eig_of_chrom[c] in [0, n_eig), the pair chromosome c is
 * scanned with: one pair per chromosome and the identity map for leave-one-chromosome-out, one pair for an overall
 * kinship.  Z is double[n][cz], the covariates themselves with the intercept first (not a basis: the weights change it
 * per phenotype); cz <= 16.  On the device, by one f64 MFMA kernel with K = n in one chain per entry:
 *   Z*_e = U_e' Z;  R_m = U_e' D[:, m, 0:H-1] for every grid point m of the chromosomes mapped to e, kept as
 *   [M][Hp][n_ld] (gbrs_scan_prepare's layout).
 * GBRS_ERR_INVALID for cz < 1 or cz > 16, n <= cz + H - 1, n > 4096, n_eig < 1 or > n_chrom, a map entry outside
 * [0, n_eig), a value of Z, U or lambda that is not finite (the message names the entry), and an eigenvalue that is not
 * above 1e-10 of its decomposition's largest (the message names the decomposition: the cohort has fewer independent
 * dosage columns than samples).  Such a refusal, and a failure after the checks, leaves the handle as it was, an earlier
 * preparation included.  An append drops the preparation and the kinship products, as it drops W.  gbrs_scan_prepare and
 * this preparation are independent: a handle may hold both, and neither changes the other's bits. */
int gbrs_scan_lmm_prepare(gbrs_scan_t *scan, int cz, const double *Z /* [n][cz] */, int n_eig, const double *const *U,
                          const double *const *lambda, const int32_t *eig_of_chrom /* [n_chrom] */);

/* P phenotypes under the prepared mixed model: pheno is double[n][P].  A caller should subtract each column's mean before
 * the call (gbrs_amd does): the model is the same, the intercept absorbs it, and y' O y - b' A^-1 b below loses fewer
 * digits; a constant column goes in as zeros.  Per (phenotype p, decomposition e), y* = U_e' y and the null fit by REML:
 * for h in [0, 1]
 *   v_i = h lambda_i + 1 - h,  o_i = 1 / v_i,  A = Z*' O Z*,  b = Z*' O y*,  rss = y*' O y* - b' A^-1 b,
 *   f(h) = (n - cz) log rss + sum log v_i + log det A  (+inf where rss <= 0),
 * minimised by a search whose steps are fixed: f at k / 20, k = 0 .. 20, the lowest wins and the lowest k among equals;
 * the bracket is its two neighbours clipped to [0, 1]; exactly 48 golden-section steps, the left point staying on equal
 * f; then the bracket's midpoint, unless the bracket still touches 0 or 1 and f there is not above f at the midpoint:
 * boundary optima are exactly 0.0 or 1.0.  hsq[p][e] is the result and sigma2[p][e] = rss / (n - cz) at it.  With hsq_in
 * (double[P][n_eig], every value in [0, 1]) the search is skipped.  rss <= 0 at h = 0 (the column of zeros): hsq 0,
 * sigma2 0 and LODs 0.0.  Then the weighted scan at the h found, with w = v^-1/2:
 *   y^ = w . y*,  Z^ = w . Z*,  X^_m = w . R_m;  Qz = Z^ after modified Gram-Schmidt in column order, each column swept
 *   twice over the ones before it and then normalised;  y~ = y^ - Qz Qz' y^,  rss0 = |y~|^2;
 *   X~ = X^_m - Qz Qz' X^_m,  G = X~' X~,  the Cholesky factor with gbrs_scan_prepare's skip rule (both of its lines),
 *   ess = |L^-1 X~' y~|^2 over the kept columns,  lod[p][m] = (n / 2) log10(rss0 / (rss0 - ess)) with gbrs_scan_run's
 *   two edge rules, and the peaks by its first-index rule.
 * lod double[P][M], peak_lod double[P][n_chrom], peak_index int64[P][n_chrom], hsq and sigma2 double[P][n_eig]; every
 * output nullable.  The phenotypes pass in chunks of 512; no W is formed: a workgroup owns a grid point and walks 64
 * phenotypes.  Every sum over the samples is one wavefront's in gbrs_scan_prepare's order: a phenotype's numbers are the
 * same bits alone or among others, at any column, in any chunk, and however the cohort was appended.  GBRS_ERR_INVALID
 * before gbrs_scan_lmm_prepare, for P < 1, for a phenotype value that is not finite (the message names the entry) and
 * for a value of hsq_in outside [0, 1]; the outputs are untouched on such a failure.  The call allocates and frees its
 * own buffers: what the handle holds, gbrs_scan_run's bits and gbrs_scan_info_t are as before.  No permutations or
 * mediation under the mixed model, REML only, additive covariates only; the SNP tests under the mixed model are
 * gbrs_scan_lmm_snps, the founder effects gbrs_scan_lmm_effects and the support intervals gbrs_scan_lmm_run_support. */
int gbrs_scan_lmm_run(gbrs_scan_t *scan, int64_t P, const double *pheno, const double *hsq_in /* [P][n_eig], nullable */,
                      double *lod, double *peak_lod, int64_t *peak_index, double *hsq /* [P][n_eig] */, double *sigma2);

/* The smallest and the largest number of kept columns over the grid points, per phenotype of the last gbrs_scan_lmm_run:
 * int32[P] each, nullable.  (The weights depend on the phenotype, so there is no rank[m] as gbrs_scan_info has it.) */
int gbrs_scan_lmm_ranks(gbrs_scan_t *scan, int32_t *rank_min, int32_t *rank_max);

typedef struct gbrs_scan_lmm_info {
    int32_t  cz, n_eig;          /* of the last gbrs_scan_lmm_prepare (0: not prepared)                          */
    int64_t  P;                  /* of the last gbrs_scan_lmm_run (0: none yet)                                  */
    double   last_kinship_ms;    /* device time of the last gbrs_scan_kinship: the products, if formed, and the sum */
    double   last_rotate_ms;     /* device time of the last preparation's rotations                              */
    double   last_null_ms;       /* of the last run: the null fits, summed over the chunks                       */
    double   last_point_ms;      /* of the last run: the weighted scan's kernel, summed over the chunks          */
    double   last_run_ms;        /* of the last run: its kernels and copies, all chunks                          */
    uint64_t device_bytes;       /* what the kinship products and the preparation hold on the device             */
    uint64_t peak_device_bytes;  /* what the handle held during the last run, the call's own buffers included    */
} gbrs_scan_lmm_info_t;
int gbrs_scan_lmm_info(gbrs_scan_t *scan, gbrs_scan_lmm_info_t *info);

/* SNP association under the mixed model (R/qtl2's scan1snps with kinship = loco): gbrs_scan_snps' test of
 * every SNP of gbrs_scan_set_snps with the polygenic effect of gbrs_scan_lmm_prepare.  No fused multiply-add anywhere.
 * The rule, per SNP j and phenotype p:
 *   1  x_s is gbrs_scan_snp_dosage's, by the same function: the same bits.
 *   2  e = eig_of_chrom[chromosome of j], x* = U_e' x; each entry one accumulator chain over the samples in the order of
 *      the K chunks, as gbrs_scan_lmm_prepare forms R_m.
 *   3  the null fit of (p, e) is gbrs_scan_lmm_run's, by the same kernel, hsq_in honoured, the column centred by the
 *      caller: sw = v^-1/2, Qz (cz columns), y~ and rss0.
 *   4  the columns g = sw . y~,  o = sw . sw,  c_k = sw . Qz_k.
 *   5  b = sum_i x*_i g_i,  raw = sum_i (x*_i x*_i) o_i,  qtx_k = sum_i x*_i c_k,i: each one chain over the samples in
 *      ascending K-chunk order (f64 MFMA, chunks of 32) that depends on the SNP's row and the phenotype's column alone.
 *   6  S = 0.0; for k ascending: S += qtx_k * qtx_k;  G = raw - S.  The pair is used iff G > 0 and G > 1e-10 raw
 *      (gbrs_scan_snps' threshold and meaning);  ess = b * b / G, a true division;  lod = (n / 2) log10(rss0 /
 *      (rss0 - ess)) with gbrs_scan_run's two edge rules.  A pair that is not used gives exactly 0.0, and the column of
 *      zeros (rss0 = 0) gives 0.0 everywhere.
 *   7  peak_lod[p][c], peak_index[p][c]: the largest LOD over the used SNPs of chromosome c and its index in handle
 *      order, the lowest on ties; NaN and -1 when there is none.  n_used[p][c] counts the used SNPs.
 * G is a difference of sums by the rule.  `used` depends on the phenotype, because the weights do.
 * pheno double[n][P]; hsq_in double[P][n_eig] or NULL; lod double[P][M_snp], used uint8[P][M_snp], peak_lod
 * double[P][n_chrom], peak_index and n_used int64[P][n_chrom], hsq and sigma2 double[P][n_eig]; every output nullable.
 * The null fits' columns of all P stay on the device for the pass ((cz + 2) n_ld doubles per (p, e)); the SNPs pass in
 * chunks of 65,536, each rotated once.  A number is the same bits for a SNP alone or among others, in any chunk, for a
 * phenotype at any column, and however the cohort was appended.  GBRS_ERR_INVALID without SNPs on the handle, before
 * gbrs_scan_lmm_prepare, for P < 1, for a phenotype value that is not finite (the message names the entry) and for a
 * value of hsq_in outside [0, 1]; the outputs are untouched and the handle is as it was.  The call allocates and frees
 * its own buffers: gbrs_scan_run, gbrs_scan_snps and gbrs_scan_lmm_run give the same bits before and after it. */
int gbrs_scan_lmm_snps(gbrs_scan_t *scan, int64_t P, const double *pheno, const double *hsq_in /* [P][n_eig], nullable */,
                       double *lod, uint8_t *used, double *peak_lod, int64_t *peak_index, int64_t *n_used,
                       double *hsq /* [P][n_eig] */, double *sigma2);

typedef struct gbrs_scan_lmm_snp_info {
    int64_t  M_snp;              /* SNPs on the handle                                                           */
    int64_t  chunk;              /* SNPs whose rotated rows are on the device at a time                          */
    int64_t  P;                  /* of the last gbrs_scan_lmm_snps (0: none yet)                                 */
    double   last_pass_ms;       /* device time of the pass: uploads, all kernels, copies                        */
    double   last_null_ms;       /* its null fits: phenotype rotations, REML, the columns, over the chunks       */
    double   last_rotate_ms;     /* its SNP dosages and their rotation, over the SNP chunks                      */
    double   last_product_ms;    /* its product kernel, over (SNP chunk, phenotype chunk)                        */
    uint64_t column_bytes;       /* the null fits' columns and rss0 of all P that the pass kept on the device    */
    uint64_t peak_device_bytes;  /* what the handle held during the pass, the call's own buffers included        */
} gbrs_scan_lmm_snp_info_t;
int gbrs_scan_lmm_snp_info(gbrs_scan_t *scan, gbrs_scan_lmm_snp_info_t *info);

/* Founder effects at QTL peaks under the mixed model (R/qtl2's scan1coef with kinship = loco at chosen
 * points): gbrs_scan_effects' answer with the polygenic effect of gbrs_scan_lmm_prepare.  For target t - the phenotype
 * column y = column[t] in [0, P) and the grid point m = point[t] in [0, M) -, with e the decomposition of m's chromosome
 * and h the heritability of (y, e), fitted by gbrs_scan_lmm_run's search or given in hsq_in.  No fused multiply-add.
 *   sw, Qz, y~, rss0     what gbrs_scan_lmm_run's null fit leaves for (y, e): w = v^-1/2, Z^ after Gram-Schmidt, the projected y^
 *   X^_j = sw . R_m[j],  j < H-1;   raw_j = |X^_j|^2;   X~_j = X^_j - Qz Qz' X^_j
 *   G = X~' X~,  b = X~' y~
 *   L, S, r              Cholesky of G with gbrs_scan_prepare's skip rule, both lines of it; S the kept columns, r their number
 *   a = L_S^-1 b_S,      ess = |a|^2
 *   R = L_S^-1 G[S, 0:H-1]   (r x (H-1));   R[:, H-1] = -sum_{j<H-1} R[:, j], j ascending        -> r x H
 *   C = R R'             r x r, symmetric positive definite: a plain Cholesky, no skip rule
 *   effect = R' C^-1 a
 *   rss1 = max(rss0 - ess, 0)     sigma2 = rss1 / (n - cz - r)     se[h] = sqrt(sigma2) |C^-1 R[:, h]|
 *   lod = (n / 2) log10(rss0 / (rss0 - ess)) with gbrs_scan_run's two edge rules
 * The last column is gbrs_scan_effects' definition carried over: the projected weighted column of founder H-1 is minus the
 * sum of the others.  The rotated, weighted constant lies in the span of Qz, so this is what the sum constraint of the
 * dosages implies, and it keeps the rule defined where a row does not add up.  effect is the minimum-norm generalised
 * least-squares solution over all H founder columns (zero-sum at full rank); a founder j < H-1 without dosage at m gets
 * exactly 0.0 with se 0.0; founders with identical dosages get identical bits; with r = 0 every effect, se and the LOD are
 * 0.0 and sigma2 stays the null model's, rss0 / (n - cz), as the formula gives it; a column of zeros gives hsq 0, effects 0.0 and lod 0.0.  sigma2 is the residual variance on the whitened scale, the
 * s2 of gbrs_scan_lmm_run's model.  The sums over the samples are gbrs_scan_lmm_run's in its order, so lod[t] carries the
 * bits of its lod[column[t]][point[t]] when both are called the same way (both fitted, or both given the same hsq_in), and
 * hsq[t] the bits of its hsq[column[t]][e].
 * pheno is double[n][P], centred as for gbrs_scan_lmm_run; hsq_in double[P][n_eig] or NULL; effect and se double[T][H], lod,
 * sigma2 and hsq double[T], rank int32[T] (the kept columns r); every output nullable.  The columns that some target names
 * are compacted on the host and pass in chunks of 512 through gbrs_scan_lmm_run's rotation and null fits - every
 * decomposition of a used column -; a chunk's targets follow in chunks of 512, one workgroup each.  A target's numbers are
 * the same bits alone or among others, at any place in the list, in any chunk, for any P and any position of its column,
 * given twice, and however the cohort was appended.  GBRS_ERR_INVALID before gbrs_scan_lmm_prepare, for P < 1 or T < 0, for
 * a column outside [0, P) or a point outside [0, M), for a phenotype value that is not finite (the message names the entry)
 * and for a value of hsq_in outside [0, 1]; the outputs are untouched and the handle is as it was.  T = 0 is GBRS_OK and
 * writes nothing.  The call allocates and frees its own buffers: gbrs_scan_run, gbrs_scan_lmm_run and gbrs_scan_lmm_snps
 * give the same bits before and after it.  No BLUP shrinkage, no effects at SNPs, no Bayes credible interval. */
int gbrs_scan_lmm_effects(gbrs_scan_t *scan, int64_t P, const double *pheno /* [n][P] */,
                          const double *hsq_in /* [P][n_eig], nullable */, int64_t T, const int64_t *column /* [T], in [0,P) */,
                          const int64_t *point /* [T], in [0,M) */, double *effect /* [T][H] */, double *se /* [T][H] */,
                          double *lod /* [T] */, double *sigma2 /* [T] */, int32_t *rank /* [T] */, double *hsq /* [T] */);

typedef struct gbrs_scan_lmm_effects_info {
    int64_t  T, P;               /* of the last gbrs_scan_lmm_effects with T > 0 (0: none yet)                   */
    int64_t  columns;            /* the distinct phenotype columns its targets named: the columns that were fitted */
    double   last_pass_ms;       /* device time of the pass: uploads, all kernels, copies                        */
    double   last_null_ms;       /* its null fits: phenotype rotations and REML, over the column chunks          */
    double   last_target_ms;     /* its target chunks: uploads, the effects kernel, copies                       */
    uint64_t peak_device_bytes;  /* what the handle held during the pass, the call's own buffers included        */
} gbrs_scan_lmm_effects_info_t;
int gbrs_scan_lmm_effects_info(gbrs_scan_t *scan, gbrs_scan_lmm_effects_info_t *info);

/* gbrs_scan_lmm_run with LOD support intervals (R/qtl2's lod_int on a scan with kinship): the pass of
 * gbrs_scan_lmm_run - the same kernels, the same bits in lod, peak_lod, peak_index, hsq, sigma2 and gbrs_scan_lmm_ranks -
 * and gbrs_scan_run_support's kernel after the peaks on each chunk's LOD rows while they are on the device.  support_lo
 * and support_hi are int64[P][n_chrom] by gbrs_scan_run_support's rule, nullable, -1 for a chromosome without points.
 * GBRS_ERR_INVALID for a drop that is negative or not finite; the other refusals are gbrs_scan_lmm_run's, and the outputs
 * are untouched on failure.  The two tables of a chunk are the call's own. */
int gbrs_scan_lmm_run_support(gbrs_scan_t *scan, int64_t P, const double *pheno, const double *hsq_in /* nullable */, double drop,
                              double *lod, double *peak_lod, int64_t *peak_index, double *hsq, double *sigma2,
                              int64_t *support_lo, int64_t *support_hi /* [P][n_chrom] */);

/* Interactive covariates (R/qtl2's scan1 with intcovar): the scan of a QTL x covariate model.  k >= 1
 * interactive covariates zint double[n][k] are used as given, not centred; the caller guarantees that each lies in the span
 * of qz (it is one of the covariates the basis was made from).  With Hx = H - 1, the columns at grid point m are, in order,
 *   additive      x_j[s] = D[s][m][j],                        j < Hx
 *   interaction   x[s]   = D[s][m][j] zint[s][q],             q = 0 .. k-1, then j < Hx
 * and gbrs_scan_prepare's factorisation runs over all Hx (1 + k) of them in that order: raw is the squared norm of a column
 * as built, the projection on qz, the Gram matrix and the Cholesky factorisation with the skip rule (both lines of it, the
 * same 1e-10) follow.  rank_add[m] counts the kept columns among the first Hx, rank_full[m] all kept columns.  Every sum
 * over the samples is formed in gbrs_scan_prepare's order, so the additive rows of the new W carry the bits of its W and
 * rank_add those of its rank for the same qz.
 * W is kept as [M * HPI][n_ld]: a point's first Hp rows as gbrs_scan_prepare lays them out, the k Hx interaction rows from
 * row Hp, zeros up to HPI, the smallest of 16, 32 and 64 that holds Hp + k Hx.  Hp + k Hx > 64 is GBRS_ERR_UNSUPPORTED.
 * The preparation is independent of gbrs_scan_prepare and of gbrs_scan_lmm_prepare and keeps its own copy of qz; an append
 * drops it.  GBRS_ERR_INVALID for k < 1, c < 1 or c > 64, n <= c + Hx (1 + k) and a value of qz or zint that is not finite
 * (the message names the entry); such a refusal leaves the handle as it was, an earlier preparation included.  A failure
 * after these checks leaves it without one. */
int gbrs_scan_int_prepare(gbrs_scan_t *scan, int c, const double *qz /* [n][c] */, int k, const double *zint /* [n][k] */);

/* P phenotypes under the prepared interaction model: pheno is double[n][P].  Per phenotype and grid point, with y~ and rss0
 * as gbrs_scan_run forms them (the same kernel),
 *   ess_add  = sum over the additive rows j of (W_j y~)^2           the bits of gbrs_scan_run's ess
 *   ess_x    = the same sum over the interaction rows,   ess_full = ess_add + ess_x   (so ess_full >= ess_add exactly)
 *   lod_full = (n / 2) log10(rss0 / (rss0 - ess_full)),  lod_add = (n / 2) log10(rss0 / (rss0 - ess_add)),
 *              each with gbrs_scan_run's two edge rules; lod_add carries the bits of gbrs_scan_run's lod for the same qz
 *   lod_int  = (n / 2) log10(rss_add / rss_full) with rss_add = rss0 - ess_add, rss_full = rss0 - ess_full;
 *              0.0 where rss0 == 0 or rss_add <= 0; +inf where rss_full <= 0 < rss_add.  Never negative, never NaN.
 * lod_full, lod_add and lod_int are double[P][M].  peak_full and peak_full_index [P][n_chrom] are gbrs_scan_run's peaks of
 * lod_full (the first of the largest per chromosome; NaN and -1 without points), peak_full_add is lod_add at that index;
 * peak_int and peak_int_index are the peaks of lod_int.  Every output is nullable, and a LOD row is formed only where an
 * output needs it.  The phenotypes pass in chunks of 512 columns; a phenotype's numbers are the same bits alone or among
 * others, at any column, in any chunk, with any subset of the outputs, and however the cohort was appended.  A column in
 * the covariates' span is the caller's to send as zeros, as for gbrs_scan_run.  GBRS_ERR_INVALID before
 * gbrs_scan_int_prepare, for P < 1 and for a value that is not finite (the message names the entry); the outputs are
 * untouched on failure.  The call allocates and frees its own buffers: gbrs_scan_run gives the same bits before and after.
 * No permutations, SNP association, mediation, effects or mixed model with interactions. */
int gbrs_scan_int_run(gbrs_scan_t *scan, int64_t P, const double *pheno /* [n][P] */,
                      double *lod_full, double *lod_add, double *lod_int,                   /* [P][M], each nullable */
                      double *peak_full, int64_t *peak_full_index, double *peak_full_add,   /* [P][n_chrom] */
                      double *peak_int, int64_t *peak_int_index);                           /* [P][n_chrom] */

typedef struct gbrs_scan_int_info {
    int64_t  n, M;               /* samples appended, grid points                                                */
    int32_t  H, c;               /* founders; covariate columns of the last gbrs_scan_int_prepare (0: not prepared) */
    int32_t  k, HPI;             /* its interactive covariates and the rows of W per grid point (16, 32 or 64)   */
    double   last_prepare_ms;    /* device time of the last gbrs_scan_int_prepare's kernel                       */
    double   last_run_ms;        /* device time of the last gbrs_scan_int_run: its kernels and copies, all chunks */
    double   last_product_ms;    /* of that, the product kernel alone, summed over the chunks                    */
    uint64_t device_bytes;       /* what the preparation holds on the device (0: not prepared)                   */
} gbrs_scan_int_info_t;
/* rank_full and rank_add are int32[M] of the last preparation, nullable; untouched when the handle has none. */
int gbrs_scan_int_info(gbrs_scan_t *scan, gbrs_scan_int_info_t *info, int32_t *rank_full, int32_t *rank_add);

/* ------------------------------------------------------------------------------------------
 * Report text (host side, no device work): the `locus <haplotypes> total [notes]` tables of
 * EMfactory.report_read_counts / report_depths (emase/EMfactory.py:289-380).
 * ---------------------------------------------------------------------------------------- */

/* One double in the form str(numpy.float64) / repr(float) give it (shortest round-trip digits, fixed
 * notation for 1e-4 <= |x| < 1e16, otherwise d.ddde+XX).  out needs 32 bytes; returns the length. */
int gbrs_format_double(double v, char *out32);

/* Writes `header_line` and then, for k = 0 .. n_rows-1 and r = order ? order[k] : k, the line
 *     name r  TAB  value(r, 0) TAB ... TAB value(r, n_cols-1)  TAB  totals[r]  [TAB note r]  LF
 * with value(r, c) = values[r * row_stride + c * col_stride] (strides in elements, so both the
 * (H x L) row-major matrix of gbrs_em_get and its transpose are taken as they lie in memory);
 * totals[r] is the caller's column sum (kept outside so that its summation order stays the
 * caller's); names / notes are byte blobs addressed by n_rows + 1 offsets, name r =
 * names[name_off[r] .. name_off[r+1]); notes / note_off may both be NULL. */
int gbrs_write_locus_table(const char *path, const char *header_line, const double *values, int64_t n_rows,
                           int32_t n_cols, int64_t row_stride, int64_t col_stride, const double *totals,
                           const char *names, const int64_t *name_off, const char *notes,
                           const int64_t *note_off, const int64_t *order);

/* HDF5 chunk decoding for the EMASE reader (emase/Sparse3DMatrix.py:80-92 reads the h<k>/indices arrays through
 * PyTables one array at a time): the chunks of a 1-D dataset, located by the caller with
 * H5Dget_chunk_info (file address, stored size, first element, filter mask), are read with pread and
 * inflated (+ un-shuffled) on `threads` threads (0 = all cores) straight into `out`.  shuffle_pos /
 * deflate_pos are the positions of those filters in the dataset's pipeline, -1 when absent. */
int gbrs_decode_chunks(const char *path, int64_t n_chunks, const uint64_t *file_addr, const uint64_t *stored_bytes,
                       const uint64_t *elem_start, const uint32_t *filter_mask, uint64_t chunk_elems,
                       uint32_t elem_size, uint64_t n_elems, int32_t shuffle_pos, int32_t deflate_pos, void *out,
                       int32_t threads);
/* 1 = libdeflate, 2 = zlib, 0 = neither could be loaded at run time. */
int gbrs_inflate_backend(void);

/* The length table of EMfactory.prepare (emase/EMfactory.py:60-94) parsed natively: text is the whole
 * file (`<locus>_<haplotype> TAB <length>` lines, plain `<locus>` keys when n_haps == 1), names / haps
 * are byte blobs with n + 1 offsets, eff_out is (n_haps x n_loci) row-major and receives
 * max(length - read_length + 1, 1) for the listed pairs (other elements untouched).  Returns 0 when
 * every line was plain, 1 when some line needs the caller's own permissive line-by-line parsing and
 * error reporting (unknown name, second underscore, a number in a form from_chars does not take). */
int gbrs_parse_length_table(const char *text, int64_t text_len, const char *names, const int64_t *name_off,
                            int64_t n_loci, const char *haps, const int64_t *hap_off, int32_t n_haps,
                            double read_length, double *eff_out);

/* The genotype call table of `gbrs quantify -G` (gbrs/emase_utils.py:262-268) parsed natively: text is the whole file
 * (`#` lines that open it are skipped, then `<gene> TAB <call>[ TAB ...]` lines, every character of a call a
 * haplotype name); gene_names / haps are byte blobs with n + 1 offsets.  Per gene g (caller zeroes / presets the
 * arrays): gene_bits[g] |= the haplotype bits of each of its lines (the reference's mask accumulates over lines),
 * gene_call[g * call_width ...] = the call of its last line, zero padded, gene_last_line[g] = that line's index
 * (what the notes keep; -1 preset = no call).  n_lines receives the number of data lines.  Returns 0 when every
 * line was plain, 1 when some line needs the caller's own permissive line-by-line parsing and error reporting
 * (unknown gene or haplotype letter, a line without a second field, bytes outside printable ASCII, a call longer
 * than call_width). */
int gbrs_parse_genotype_table(const char *text, int64_t text_len, const char *gene_names, const int64_t *gene_off,
                              int64_t n_genes, const char *haps, const int64_t *hap_off, int32_t n_haps,
                              uint32_t *gene_bits, char *gene_call, int32_t call_width, int32_t *gene_last_line,
                              int64_t *n_lines);

/* The numbers of a `label TAB v1 TAB ... TAB vn` table (the genes.tpm report `gbrs reconstruct` reads,
 * gbrs/gbrs_utils.py:450-459): text holds exactly n_rows such lines (header removed), out receives n_rows x n_cols
 * doubles.  Returns 0, or 1 when a line is not of that plain form (the caller then parses it its own way). */
int gbrs_parse_number_table(const char *text, int64_t text_len, int64_t n_rows, int32_t n_cols, double *out);

/* `.npz` inputs of `gbrs reconstruct` (gbrs/gbrs_utils.py:420-441 opens avecs.npz with numpy.load and reads one
 * member per gene, :490 - zipfile re-parses the member's header and CRC-checks it on every access).
 * gbrs_zip_directory reads the central directory of a zip image (buf/len = the mapped file) once: member k's
 * compression method (0 stored, 8 deflate), compressed and plain sizes and local-header offset, and the member
 * names as one blob with an LF after each name.  Arrays hold `cap` members and `names_cap` bytes; the member count
 * and the blob size come back in n_members / names_len, so a first call with cap = 0 sizes the second.
 * GBRS_ERR_UNSUPPORTED: multi-disk archive (the caller falls back to zipfile). */
int gbrs_zip_directory(const uint8_t *buf, uint64_t len, uint64_t cap, uint16_t *method, uint64_t *csize,
                       uint64_t *usize, uint64_t *header_off, uint32_t *crc32 /* nullable: the members' CRC-32 */,
                       char *names, uint64_t names_cap, uint64_t *n_members, uint64_t *names_len);
/* n members' plain contents (their .npy images), member k into out[k] (usize[k] bytes, caller allocated), copied or
 * inflated on `threads` threads (0 = all cores), largest member first.  crc32 (nullable): the members' CRC-32 from the
 * central directory, checked on the thread that produced the bytes - numpy.load / zipfile check every member and raise
 * BadZipFile (the reference inherits that at gbrs_utils.py:420-441); a mismatch returns GBRS_ERR_INVALID. */
int gbrs_zip_read_members(const uint8_t *buf, uint64_t len, int64_t n, const uint64_t *header_off, const uint16_t *method,
                          const uint64_t *csize, const uint64_t *usize, const uint32_t *crc32, uint8_t *const *out,
                          int32_t threads);
/* n equally shaped .npy members (the per-gene 8 x 8 blocks) -> out[k * item_bytes ...], on `threads` threads
 * (0 = all cores): a member whose .npy image is exactly npy_header followed by item_bytes of data is copied
 * (stored) or inflated (raw deflate) into place; any other member - and, with crc32 given, one that fails its CRC-32 -
 * gets needs_fallback[k] = 1 and is left to the caller. */
int gbrs_npz_stack(const uint8_t *buf, uint64_t len, int64_t n, const uint64_t *header_off, const uint16_t *method,
                   const uint64_t *csize, const uint64_t *usize, const uint32_t *crc32, const uint8_t *npy_header,
                   uint64_t npy_header_len, uint64_t item_bytes, uint8_t *out, uint8_t *needs_fallback, int32_t threads);

#ifdef __cplusplus
}
#endif
#endif /* GBRS_HIP_H */
