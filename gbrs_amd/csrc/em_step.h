// What one pass over an EM handle launches (em.hip): the E-step kernel instance, the long-row kernel, how much of `acc` the
// gather writes, the M-step kernel and where the error pass goes - resolved by a pure function from what is known once the
// layout is built and the kind of pass, once per API call.  Host only, like em_plan.h (tests/native/em_step_driver.cpp).
#pragma once

#include "em_plan.h"

namespace gbrs {

struct EmStepShape {              // a handle after gbrs_em_create*
    bool tiled = false;           // the tile layout; false: the CSC kernels
    uint32_t H = 0;
    uint32_t tH = 0, view = 1;    // the layout's haplotypes per (half-)locus (EmPlan)
    bool no_tiles = true, no_long = true, no_entries = true;   // TileLayout::n_tiles, n_long and N are zero
    bool weighted = false, deterministic = false, all_one_word = false;   // TileLayout's
    uint32_t persist_groups = 0;
    bool acc_handed_out = false;  // a partial entry point has given `acc` to the caller, who all-reduces all of it from then on
    bool no_fused_mstep = false;  // EmTuning's
};

enum class EmPass {
    Prepare,   // theta taken as ones, every element of acc written
    Step,      // one model-4 iteration
    Partial,   // an E-step whose acc the caller all-reduces (gbrs_em_prepare_partial's M-step half, gbrs_em_estep_partial)
    Model,     // models 1-3: their own E-step kernels (em_models.inc), then the common M-step
};
enum class EmEstep { None, Csc, Tiles, TilesOneWord, TilesDeterministic, Persistent, PersistentOneWord, Models };
enum class EmLongRows { None, Atomic, Serial };
enum class EmGather { None, Written, All };      // none: the CSC and model kernels write acc themselves, or the fused kernel follows
enum class EmMstep { Fused, Elem, PerLocus };    // with the gather in one launch / one thread per element / per locus

struct EmStepRoute {
    EmPass pass = EmPass::Step;
    EmEstep estep = EmEstep::None;       // none: no tile (no entry) to launch for
    int width = 0;                       // tile kernels: the haplotype count they are compiled for, 0 the run-time count
    bool weighted = false;
    EmLongRows long_rows = EmLongRows::None;
    EmGather gather = EmGather::None;
    EmMstep mstep = EmMstep::PerLocus;
    bool mstep_adds_extra = false;       // the long rows' sums are still in acc_extra when the M-step reads acc
    bool counts_stale = false;           // the M-step does not store the expected counts (em_refresh_counts makes them)
    bool err_rides = false;              // a pending error pass runs on the tile launch; false: on a launch of its own, before
    bool err_defer = false;              // this pass's own error pass may be left pending for the next one
};

#if defined(GBRS_NO_ONEWORD)
constexpr bool EM_ONEWORD_TILES = false;
#else
constexpr bool EM_ONEWORD_TILES = true;
#endif

inline EmStepRoute em_step_route(const EmStepShape &s, EmPass pass) {
    EmStepRoute r;
    r.pass = pass;
    const bool ones = pass == EmPass::Prepare;
    r.mstep = (s.H & (s.H - 1)) == 0 ? EmMstep::Elem : EmMstep::PerLocus;
    if (pass == EmPass::Model) {
        r.estep = EmEstep::Models;
        return r;
    }
    if (!s.tiled) {
        r.estep = s.no_entries ? EmEstep::None : EmEstep::Csc;
        return r;
    }
    const uint32_t tH = s.tH;
    r.width = (tH == 1 || tH == 2 || tH == 4 || tH == 8 || tH == 16) ? (int)tH : 0;
    r.weighted = s.weighted;
    const bool one_word = r.width == 8 && !s.weighted && s.all_one_word;
    if (s.no_tiles) r.estep = EmEstep::None;
    else if (!ones && !s.deterministic && s.persist_groups > 0 && r.width >= 1 && r.width <= 8)
        r.estep = one_word ? EmEstep::PersistentOneWord : EmEstep::Persistent;
    else if (s.deterministic) r.estep = EmEstep::TilesDeterministic;
    else if (EM_ONEWORD_TILES && one_word) r.estep = EmEstep::TilesOneWord;
    else r.estep = EmEstep::Tiles;
    r.err_rides = !ones && !s.no_tiles;
    if (!s.no_long) r.long_rows = s.deterministic ? EmLongRows::Serial : EmLongRows::Atomic;
    // (half-locus view: the fused kernel's per-locus totals would be per half; gather and M-step stay two launches there)
    const bool fused = pass == EmPass::Step && r.mstep == EmMstep::Elem && !s.acc_handed_out && s.view == 1 && !s.no_fused_mstep;
    const bool all = pass != EmPass::Step || s.acc_handed_out || (tH & (tH - 1)) != 0 || s.view > 1;
    r.gather = fused ? EmGather::None : all ? EmGather::All : EmGather::Written;
    if (fused) r.mstep = EmMstep::Fused;
    r.mstep_adds_extra = r.gather == EmGather::Written && !s.no_long;
    r.counts_stale = fused;
    r.err_defer = !ones;
    return r;
}

// The gather-side M-step (em_layout.h, GatherArgs): a third way to run a Model-4 step on the tile layout, beside "fused
// gather + M-step launch" and "two launches".  Iteration n's M-step is applied by launch n + 1's tile prologues and a plain
// elementwise M-step closes an API call; no slot rows, no gather, one launch per iteration.  Which passes take it is
// decided here, beside the route and from the same shape, by what the route does not know:
struct EmGatherShape {
    bool no_heavy = true;         // TileLayout::n_heavy is zero: no locus has more than HEAVY_SLOTS slots
    uint32_t n_tiles = 0, tile_waves = 0, msum_cap = 0;   // the block sums take tile_waves slots per tile
    bool posterior = false, resample = false, pair_mode = false;   // GBRS_EM_POSTERIOR, GBRS_EM_RESAMPLE, gbrs_em_pair_begin
};

inline bool em_gather_mstep(const EmStepShape &s, const EmGatherShape &g, EmPass pass, const EmTuning &t) {
    if (pass != EmPass::Step || !s.tiled || s.no_tiles) return false;
    const EmStepRoute r = em_step_route(s, pass);
    if (r.estep != EmEstep::Tiles && r.estep != EmEstep::TilesOneWord) return false;     // not deterministic, not persistent
    if (s.weighted) return false;
    if (!(s.H == 1 || s.H == 2 || s.H == 4 || s.H == 8) || s.tH != s.H || s.view != 1) return false;
    if (!s.no_long || !g.no_heavy) return false;
    if (s.acc_handed_out) return false;
    if (g.posterior || g.resample || g.pair_mode) return false;
    if ((uint64_t)g.n_tiles * g.tile_waves > g.msum_cap) return false;
    return !t.no_gather_mstep;
}

}  // namespace gbrs
