// Prints whether a pass over an EM handle takes the gather-side M-step (gbrs_amd/csrc/em_step.h, em_gather_mstep): the plan
// of em_plan.h under the GBRS_TUNING_* variables of this process' environment, the facts of the built layout and of the
// handle as given (tests/test_em_gather_route_cpu.py).  Host C++ only.
//   em_gather_driver <H> <L> <N> <flags> <counts given 0|1> <pass> <n_tiles> <n_long> <all_one_word 0|1>
//                    <acc handed out 0|1> <n_heavy> <msum_cap> <pair mode 0|1>
// pass: prepare | step | partial | model
#include "../../gbrs_amd/csrc/em_step.h"

#include <cstdio>
#include <cstring>

using namespace gbrs;

int main(int argc, char **argv) {
    if (argc != 14) return 2;
    EmShape sh;
    sh.H = (uint32_t)std::atoi(argv[1]);
    sh.L = (uint32_t)std::atoll(argv[2]);
    sh.R = sh.N = (uint64_t)std::atoll(argv[3]);
    sh.flags = (uint32_t)std::atoi(argv[4]);
    sh.counts_given = std::atoi(argv[5]) != 0;
    sh.n_cu = 256;
    sh.tile_words = 2048; sh.tile_words_max = 32768 - 64;
    sh.dict = sh.dict_half = {32, 1024, 3072, 48};
    const EmTuning t = em_tuning_from_env();
    const EmPlan p = em_plan(sh, t);
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
    EmGatherShape g;
    g.no_heavy = std::atoll(argv[11]) == 0;
    g.n_tiles = (uint32_t)std::atoll(argv[7]);
    g.tile_waves = 8;
    g.msum_cap = (uint32_t)std::atoll(argv[12]);
    g.posterior = (sh.flags & GBRS_EM_POSTERIOR) != 0;
    g.resample = (sh.flags & GBRS_EM_RESAMPLE) != 0;
    g.pair_mode = std::atoi(argv[13]) != 0;
    const EmStepRoute before = em_step_route(s, (EmPass)pass);
    const bool taken = em_gather_mstep(s, g, (EmPass)pass, t);
    const EmStepRoute after = em_step_route(s, (EmPass)pass);       // the decision leaves the route alone
    const bool same = before.estep == after.estep && before.gather == after.gather && before.mstep == after.mstep;
    std::printf("gather_mstep=%d no_gather_mstep=%d plan_no_gather_mstep=%d route_unchanged=%d\n", (int)taken, (int)t.no_gather_mstep,
                (int)p.no_gather_mstep, (int)same);
    return 0;
}
