// Prints the route gbrs_amd/csrc/hmm_route.h resolves for one handle shape under the GBRS_TUNING_HMM_* variables of
// this process' environment (tests/test_hmm_route_cpu.py).  Host C++ only.
//   hmm_route_driver <founders> <n_samples> <n_chrom> <total_trans>
#include "../../gbrs_amd/csrc/hmm_route.h"

#include <cstdio>

using namespace gbrs;

int main(int argc, char **argv) {
    if (argc != 5) return 2;
    const int H = std::atoi(argv[1]);
    const HmmShape shape{H * (H + 1) / 2, H, std::atoi(argv[2]), std::atoi(argv[3]), std::atoll(argv[4])};
    // what gbrs_hmm_set_expression and gbrs_hmm_run do, in their order
    const bool deferred = hmm_defers_emission(shape, hmm_tuning_from_env(), H == 8 && shape.n_samples >= 4);
    const HmmTuning t = hmm_tuning_from_env();
    const HmmRoute r = hmm_route(shape, t, deferred);
    static const char *sweep[] = {"generic", "quad", "wave", "blocked", "mfma"};
    static const char *delta[] = {"with_sweep", "wave", "lanes", "blocked_rank", "blocked_ops"};
    static const char *bp[] = {"with_sweep", "chains", "quad", "wave", "lanes", "generic"};
    std::printf("sweep=%s delta=%s bp=%s batched=%d mfma_groups=%d deferred=%d grouped=%d delta_interleaved=%d xcd_mask=%d xcd_span=%d "
                "tie_check=%d tol_abs=%g tol_rel=%g serial=%d back_after=%d bp_after=%d delta_after_ops=%d free_backward=%d "
                "block_genes=%d blocks_max=%d head=%d pipe_first=%d\n",
                sweep[(int)r.sweep], delta[(int)r.delta], bp[(int)r.bp], (int)r.batched, r.mfma_groups, (int)deferred, (int)r.grouped,
                (int)r.delta_interleaved, r.xcd_mask, r.xcd_span, (int)r.tie_check, r.tol_abs, r.tol_rel, (int)r.serial,
                (int)r.back_after, (int)r.bp_after, (int)r.delta_after_ops, (int)r.free_backward(), t.block_genes, t.blocks_max,
                t.head_pct, t.pipe_first_pct);
    return 0;
}
