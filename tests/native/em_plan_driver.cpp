// Prints the plan gbrs_amd/csrc/em_plan.h resolves for one EM handle under the GBRS_TUNING_* variables of this process'
// environment, and what its data-dependent rules answer (tests/test_em_plan_cpu.py).  Host C++ only.
//   em_plan_driver <H> <L> <R> <N> <flags> <counts given 0|1> <n_cu> [rule ...]
// rules:  tile=<words>   fold=<words_in>,<folded>   whole=<P>,<P2>,<L>,<V>   group=<P>,<P2>   fit=<V>,<L>
#include "../../gbrs_amd/csrc/em_plan.h"

#include <cstdio>
#include <cstring>

using namespace gbrs;

// the constants of em_layout.h (a HIP header), restated: what em.hip passes in
static EmDictLimits limits(bool weighted, unsigned H) {
    const unsigned pos_bits = H <= 8 ? 5 : 3, lds = weighted ? 4608 : (H == 16 ? 4800 : 3072);
    return {1u << pos_bits, 1u << (32 - H - 2 * pos_bits), lds, ((lds + 64) / 8 - 1) / H};
}

int main(int argc, char **argv) {
    if (argc < 8) return 2;
    EmShape s;
    s.H = (uint32_t)std::atoi(argv[1]);
    s.L = (uint32_t)std::atoll(argv[2]);
    s.R = (uint64_t)std::atoll(argv[3]);
    s.N = (uint64_t)std::atoll(argv[4]);
    s.flags = (uint32_t)std::atoi(argv[5]);
    s.counts_given = std::atoi(argv[6]) != 0;
    s.n_cu = std::atoi(argv[7]);
    s.tile_words = 2048; s.tile_words_max = 32768 - 64; s.tile_rounds_min = 1;
    if (s.H <= 16) s.dict = limits(em_weighted(s.flags, s.counts_given), s.H);
    if (s.H == 16) s.dict_half = limits(false, 8);
    const EmPlan p = em_plan(s, em_tuning_from_env());
    std::printf("tiled=%d view=%u tH=%u tL=%u row_order=%d merge=%d deterministic=%d weighted=%d side_by_side=%u locus_sets=%d "
                "whole_row_sets=%d group_sets=%d group_sets_forced=%d sets_forced=%d set_min_rows=%u counted_pairs=%d fold=%d "
                "fold_mode=%d fold_forced=%d per_cu=%u places=%llu tile_words_forced=%u reorder_tiles=%d d_max=%u dseg=%u "
                "dict_room=%d persist_groups=%u lead_mask=%u resample_cut=%u",
                (int)p.tiled, p.view, p.tH, p.tL, p.row_order, (int)p.merge, (int)p.deterministic, (int)p.weighted, p.side_by_side,
                (int)p.locus_sets, (int)p.whole_row_sets, (int)p.group_sets, (int)p.group_sets_forced, p.sets_forced, p.set_min_rows,
                (int)p.counted_pairs, (int)p.fold, p.fold_mode, (int)p.fold_forced, p.per_cu, (unsigned long long)p.places,
                p.tile_words_forced, (int)p.reorder_tiles, p.d_max, p.dseg, (int)p.dict_room, p.persist_groups, p.lead_mask,
                p.resample_cut);
    for (int i = 8; i < argc; ++i) {
        unsigned long long a = 0, b = 0, c = 0, d = 0;
        if (std::sscanf(argv[i], "tile=%llu", &a) == 1) std::printf(" tile=%u", em_tile_words(p, a));
        else if (std::sscanf(argv[i], "fold=%llu,%llu", &a, &b) == 2) std::printf(" fold_taken=%d", (int)em_take_fold(p, a, b));
        else if (std::sscanf(argv[i], "whole=%llu,%llu,%llu,%llu", &a, &b, &c, &d) == 4)
            std::printf(" whole=%d", (int)em_use_whole_row_sets(p, a, b, c, d));
        else if (std::sscanf(argv[i], "group=%llu,%llu", &a, &b) == 2) std::printf(" group=%d", (int)em_use_group_sets(p, a, b));
        else if (std::sscanf(argv[i], "fit=%llu,%llu", &a, &b) == 2) std::printf(" fit=%d", (int)em_group_sets_fit(p, a, b));
        else return 2;
    }
    std::printf("\n");
    return 0;
}
