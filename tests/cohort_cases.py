"""Launch sizes at which the outputs built on top of an HMM run - grid dosages, path draws, diagnostics, log-likelihoods,
panel matching, SNP dosages and the scan's hand-over - are held to their restatements: plain numpy, no GPU.

`gbrs reconstruct --sample-file` launches `--batch-size` samples at a time, 64 unless told otherwise, and hmm_route.h
sends a 36-state pass of 64 or more samples through the MFMA sweeps, the samples-on-lanes delta chain and the
samples-on-lanes backpointers.  Each row names a handle shape and the route tests/native/hmm_route_driver.cpp prints for it
with no GBRS_TUNING_HMM_* variable set.  tests/test_cohort_sizes_cpu.py holds every row to its route on the CPU;
tests/test_cohort_sizes_gpu.py runs the rows.  A threshold that moves fails the CPU test by row: the GPU rows then have to
be aimed at the kernels again.

Which kernel a failing sample index points at - the partitions of a launch's samples:

  partition of         made by                                              65 samples give
  8  (IMPUTE_SAMPLES)  the impute kernels, one workgroup per group          8 full groups and a ninth of one sample
  16                   the MFMA sweeps' groups (a last group shadows its     4 full groups and a fifth with one real sample
                       last real sample), and what hmm_make_logs builds      and 15 shadows
                       from their bscale / invz (beta_corr_kernel)
  16 (4 * DIAG_WAVES)  diag_pair_kernel's slabs                             4 full slabs and a fifth of one sample
  16 within 64         match_cross_kernel: wavefront w of a workgroup takes  wavefronts 0 .. 3 of block 0 all real;
                       the rows 16 w .. 16 w + 15 of its block               block 1: one row, 63 shadows
  64 (MT_ROWS)         match_cross_kernel's blocks of rows (blockIdx.x)      a second block of one row
  1                    grid_kernel, sample_paths_kernel, loglik_reduce_-     slots 0 .. 64; a wrong stride shows from
                       kernel, loglik_tables_kernel, diag_gene_kernel index  the first slot it reaches
                       (sample0 + slot) * total_genes, the slot from
                       blockIdx.y / .z or a row number

So a first wrong sample of 8, 16, 24, ... points at the impute groups; 16, 32 or 48 at an MFMA group, a diagnostics slab or
a wavefront of the match; 64 at the last group / slab / block of one; any other index at a per-slot stride."""
import collections

Case = collections.namedtuple("Case", "founders n_samples sweep delta bp batched")

CASES = [
    # the smallest launch above the blocked scan: the one-sample-per-wave chains at 36 states with viterbi_bp_kernel
    Case(8, 5, "wave", "wave", "generic", 0),
    # the command's own launch: every partition exactly full
    Case(8, 64, "mfma", "lanes", "lanes", 1),
    # one past it: a fifth MFMA group and a fifth diagnostics slab with one sample, a ninth SNP group with one sample, a
    # second match block with one row
    Case(8, 65, "mfma", "lanes", "lanes", 1),
    # match only: odd H takes match_cross_kernel<false>, the scalar staging path
    Case(3, 65, "wave", "wave", "generic", 1),
]

# the first and the last member of every partition of 8, 16 and 64 that a kernel above makes; sample s of a launch is
# grid_cases.sample_problem(H, style, s), so the oracle caches of tests/grid_cases.py serve them
EDGE_SAMPLES = (0, 7, 8, 15, 16, 31, 32, 47, 48, 63, 64)

# the partition sizes the table above and EDGE_SAMPLES assume; tests/test_cohort_sizes_cpu.py reads them from the sources
PARTITIONS = {"IMPUTE_SAMPLES": 8, "DIAG_SLAB": 16, "MT_ROWS": 64}


def case_id(c):
    return f"h{c.founders}-n{c.n_samples}"


def case(founders, n_samples):
    return next(c for c in CASES if (c.founders, c.n_samples) == (founders, n_samples))


def edge_samples(n_samples):
    """EDGE_SAMPLES cut to a launch's size."""
    return tuple(s for s in EDGE_SAMPLES if s < n_samples)


def streams(n_samples):
    """Stream ids of a launch's path draws that are not the slot numbers: 2 n - slot, descending, none below n."""
    return [2 * n_samples - s for s in range(n_samples)]


# Path draws.  tests/test_sim_geno_gpu.py's rule: no draw may be left out of the comparison, so the smallest decision
# margin must stay above its FLOOR (1e-12), else another seed is chosen on the CPU.  PATH_SEED is that suite's own seed:
# the restatement alone (tests/sim_geno_restate.py on the oracle's alpha), over the EDGE_SAMPLES of the rows (8, 5) and
# (8, 65), both styles, 65 draws and the streams above - some 420,000 decisions - decides nothing by less than 1.6e-7
# with it (of the eleven seeds that follow it, none does better than 3.0e-7 and most do worse: with that many uniform
# thresholds a smallest margin near 1e-7 is what to expect).  PATH_MARGIN = 1e-7 is five orders above the floor;
# tests/test_cohort_sizes_cpu.py asserts it on the CPU, the GPU test asserts the floor on the device's own alpha.
PATH_DRAWS = (1, 65)
PATH_SEED = 0x5EED00000000 + 77
PATH_MARGIN = 1e-7
PATH_ROWS = ((8, 5), (8, 65))
STYLES = ("do", "benign")


def path_margin(seed, founders, n_samples, style):
    """The smallest decision margin of the restatement on the oracle's alpha over the row's EDGE_SAMPLES."""
    import grid_cases
    import sim_geno_restate as restate
    table = restate.change_table(founders)
    ids = streams(n_samples)
    p0 = grid_cases.problem(founders, style)
    smallest = float("inf")
    for s in edge_samples(n_samples):
        res = grid_cases.oracle_arrays(founders, style, s)[0]
        for ci, c in enumerate(p0.chroms):
            _, _, margins, degenerate = restate.sample_paths(res[c]["alpha"], p0.tprob[c], seed, ids[s], ci, max(PATH_DRAWS), table)
            assert degenerate == 0
            smallest = min(smallest, float(margins.min()))
    return smallest
