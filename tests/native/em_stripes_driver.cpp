// Prints what gbrs_amd/csrc/em_plan.h resolves about stripes for one EM handle under the GBRS_TUNING_* variables of this
// process' environment, and what its two rules answer (tests/test_em_stripes_cpu.py).  Host C++ only.
//   em_stripes_driver <H> <L> <R> <N> <flags> <counts given 0|1> <n_cu> [rule ...]
// rules:  take=<words>   pick=<forced>,<words>,<cells4>,<cells2>
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
    std::printf("counted_pairs=%d stripes_one=%d stripes_two=%d stripes_forced=%d cap_num=%u cap_den=%u", (int)p.counted_pairs,
                p.stripes_one, p.stripes_two, (int)p.stripes_forced, STRIPE_CAP_NUM, STRIPE_CAP_DEN);
    for (int i = 8; i < argc; ++i) {
        unsigned long long a = 0, b = 0, c = 0;
        int f = 0;
        if (std::sscanf(argv[i], "take=%llu", &a) == 1) std::printf(" take=%d", (int)em_take_stripes(p, a));
        else if (std::sscanf(argv[i], "pick=%d,%llu,%llu,%llu", &f, &a, &b, &c) == 4) std::printf(" pick=%u", em_stripe_pick(f, a, b, c));
        else return 2;
    }
    std::printf("\n");
    return 0;
}
