"""Sample batches whose HMM pass takes the two-samples-per-wave chains (hmm_route.h: `batched`, from HMM_BATCH_MIN = 24
samples on, until the MFMA sweeps and the samples-on-lanes kernels take over), as plain data: no import beyond the
standard library, no GPU.

Each row names a handle shape, the GBRS_TUNING_HMM_* variables to set (none: the library's defaults) and the route
tests/native/hmm_route_driver.cpp prints for them.  tests/test_hmm_route_cpu.py holds every row to its route on the CPU;
tests/test_hmm_batched_wave_gpu.py runs every row against the oracle.  A change that moves a threshold, or a new kernel
that takes these sample counts, fails the CPU test by row: the GPU rows then have to be aimed at the kernels again."""
import collections

PREFIX = "GBRS_TUNING_HMM_"

Case = collections.namedtuple("Case", "founders n_samples env sweep delta bp batched")


def _env(**short):
    return {PREFIX + k: str(v) for k, v in short.items()}


CASES = [
    # 36 states, library defaults: 24 is the first batched count (even), 25 leaves a lone sample in the last wave, at 33
    # the samples-on-lanes backpointer kernel has a partly filled group, 63 is the last count below the MFMA threshold
    Case(8, 24, {}, "wave", "wave", "generic", 1),
    Case(8, 25, {}, "wave", "wave", "generic", 1),
    Case(8, 33, {}, "wave", "wave", "lanes", 1),
    Case(8, 63, {}, "wave", "wave", "lanes", 1),
    # mixed routes within the documented thresholds: MFMA sweeps beside the batched delta chain, batched sweeps beside the
    # samples-on-lanes delta chain
    Case(8, 25, _env(MFMA=16), "mfma", "wave", "generic", 1),
    Case(8, 25, _env(MFMA=0, DLANES=16, BPLANES=5), "wave", "lanes", "lanes", 1),
    # the stream orderings
    Case(8, 25, _env(SERIAL=1), "wave", "wave", "generic", 1),
    Case(8, 25, _env(BACK_AFTER=1, BP_AFTER=1), "wave", "wave", "generic", 1),
    # 28, 10 and 6 states
    Case(7, 25, {}, "wave", "wave", "generic", 1),
    Case(4, 24, {}, "wave", "wave", "generic", 1),
    Case(4, 25, {}, "wave", "wave", "generic", 1),
    Case(3, 25, {}, "wave", "wave", "generic", 1),
    # outside the wave family (never batched): the grids of the quad and of the generic kernels at 25 samples
    Case(16, 25, {}, "quad", "with_sweep", "quad", 0),
    Case(5, 25, {}, "generic", "with_sweep", "with_sweep", 0),
]


def case_id(c):
    env = "-".join(f"{k[len(PREFIX):].lower()}{v}" for k, v in c.env.items()) or "defaults"
    return f"h{c.founders}-n{c.n_samples}-{env}"


def genes_per_chrom(founders):
    """Chromosome lengths of the GPU rows.  8 founders: chains of 0 to 6 steps around the three-set prefetch ring and its
    unrolled tail, and lengths around the backtrace chunk."""
    if founders == 8:
        return [1, 2, 3, 4, 5, 6, 7, 63, 64, 65, 129, 200]
    if founders == 16:
        return [1, 2, 3, 5, 33, 70]
    return [1, 2, 3, 4, 6, 65, 130]
