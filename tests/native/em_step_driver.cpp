// Prints the route gbrs_amd/csrc/em_step.h resolves for one pass over an EM handle: the plan of em_plan.h under the
// GBRS_TUNING_* variables of this process' environment, the facts of the built layout as given, the kind of pass
// (tests/test_em_step_route_cpu.py).  Host C++ only.
//   em_step_driver <H> <L> <N> <flags> <counts given 0|1> <pass> <n_tiles> <n_long> <all_one_word 0|1> <acc handed out 0|1>
// pass: prepare | step | partial | model
#include "../../gbrs_amd/csrc/em_step.h"

#include <cstdio>
#include <cstring>

using namespace gbrs;

int main(int argc, char **argv) {
    if (argc != 11) return 2;
    EmShape sh;
    sh.H = (uint32_t)std::atoi(argv[1]);
    sh.L = (uint32_t)std::atoll(argv[2]);
    sh.R = sh.N = (uint64_t)std::atoll(argv[3]);
    sh.flags = (uint32_t)std::atoi(argv[4]);
    sh.counts_given = std::atoi(argv[5]) != 0;
    sh.n_cu = 256;
    sh.tile_words = 2048; sh.tile_words_max = 32768 - 64;
    sh.dict = sh.dict_half = {32, 1024, 3072, 48};      // (the dictionary limits take no part in a step's route)
    const EmPlan p = em_plan(sh, em_tuning_from_env());
    static const char *const passes[] = {"prepare", "step", "partial", "model"};
    int pass = -1;
    for (int i = 0; i < 4; ++i)
        if (!std::strcmp(argv[6], passes[i])) pass = i;
    if (pass < 0) return 2;
    EmStepShape s;
    s.tiled = p.tiled;
    s.H = sh.H; s.tH = p.tH; s.view = p.view;
    s.no_tiles = std::atoll(argv[7]) == 0 || !p.tiled;
    s.no_long = std::atoll(argv[8]) == 0 || !p.tiled;
    s.no_entries = sh.N == 0;
    s.weighted = p.weighted; s.deterministic = p.deterministic;
    s.all_one_word = std::atoi(argv[9]) != 0;
    s.persist_groups = p.persist_groups;
    s.acc_handed_out = std::atoi(argv[10]) != 0;
    s.no_fused_mstep = p.no_fused_mstep;
    const EmStepRoute r = em_step_route(s, (EmPass)pass);
    static const char *const estep[] = {"none", "csc", "tiles", "tiles_one_word", "tiles_deterministic", "persistent",
                                        "persistent_one_word", "models"};
    static const char *const long_rows[] = {"none", "atomic", "serial"};
    static const char *const gather[] = {"none", "written", "all"};
    static const char *const mstep[] = {"fused", "elem", "per_locus"};
    std::printf("estep=%s width=%d weighted=%d long_rows=%s gather=%s mstep=%s mstep_adds_extra=%d counts_stale=%d err_rides=%d "
                "err_defer=%d tH=%u view=%u no_fused_mstep=%d no_float_check=%d\n",
                estep[(int)r.estep], r.width, (int)r.weighted, long_rows[(int)r.long_rows], gather[(int)r.gather],
                mstep[(int)r.mstep], (int)r.mstep_adds_extra, (int)r.counts_stale, (int)r.err_rides, (int)r.err_defer, p.tH, p.view,
                (int)p.no_fused_mstep, (int)p.no_float_check);
    return 0;
}
