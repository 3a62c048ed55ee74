// Prints what gbrs_amd/csrc/em_plan.h resolves for the tile cut of one EM handle under the GBRS_TUNING_* variables of this
// process' environment (tests/test_em_tile_cut_cpu.py).  Host C++ only.
//   em_tile_cut_driver <H> <flags> <counts given 0|1> <n_cu> <err_blocks> [rule ...]
// rules:  take=<total words>   first=<total words>   rescale=<tile words>,<tiles>   target=<places>,<side by side>,<err blocks>,<forced>
#include "../../gbrs_amd/csrc/em_plan.h"

#include <cstdio>

using namespace gbrs;

// the constants of em_layout.h (a HIP header), restated: what em.hip passes in
static EmDictLimits limits(bool weighted, unsigned H) {
    const unsigned pos_bits = H <= 8 ? 5 : 3, lds = weighted ? 4608 : (H == 16 ? 4800 : 3072);
    return {1u << pos_bits, 1u << (32 - H - 2 * pos_bits), lds, ((lds + 64) / 8 - 1) / H};
}

int main(int argc, char **argv) {
    if (argc < 6) return 2;
    EmShape s;
    s.H = (uint32_t)std::atoi(argv[1]);
    s.L = 400; s.R = 20000; s.N = 100000;
    s.flags = (uint32_t)std::atoi(argv[2]);
    s.counts_given = std::atoi(argv[3]) != 0;
    s.n_cu = std::atoi(argv[4]);
    s.err_blocks = (uint32_t)std::atoi(argv[5]);
    s.tile_words = 2048; s.tile_words_max = 32768 - 64; s.tile_rounds_min = 1;
    if (s.H <= 16) s.dict = limits(em_weighted(s.flags, s.counts_given), s.H);
    if (s.H == 16) s.dict_half = limits(false, 8);
    const EmPlan p = em_plan(s, em_tuning_from_env());
    std::printf("exact_cut=%d tile_target=%llu places=%llu side_by_side=%u tile_words=%u tile_words_cap=%u tile_words_forced=%u "
                "passes=%d d_max=%u dseg=%u",
                (int)p.exact_cut, (unsigned long long)p.tile_target, (unsigned long long)p.places, p.side_by_side, p.tile_words,
                p.tile_words_cap, p.tile_words_forced, TILE_CUT_PASSES, p.d_max, p.dseg);
    for (int i = 6; i < argc; ++i) {
        unsigned long long a = 0, b = 0, c = 0;
        long long d = 0;
        if (std::sscanf(argv[i], "first=%llu", &a) == 1) std::printf(" first=%u", em_cut_tile_words(p, a));
        else if (std::sscanf(argv[i], "take=%llu", &a) == 1) std::printf(" take=%d", (int)em_take_exact_cut(p, a));
        else if (std::sscanf(argv[i], "rescale=%llu,%llu", &a, &b) == 2) std::printf(" rescale=%u", em_cut_rescale(p, (uint32_t)a, b));
        else if (std::sscanf(argv[i], "target=%llu,%llu,%llu,%lld", &a, &b, &c, &d) == 4)
            std::printf(" target=%llu", (unsigned long long)em_tile_target(a, (unsigned)b, (uint32_t)c, (int)d));
        else return 2;
    }
    std::printf("\n");
    return 0;
}
