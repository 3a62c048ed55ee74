// What the genome scan (scan.hip) reads from an HMM handle (hmm_passes.hip): the grid dosages of the last run, on the device.
#pragma once
#include "common.h"

namespace gbrs {

struct HmmGridView {
    int device = 0, H = 0, n = 0;            // n: samples `dosage` holds (all of the run, or the one asked for)
    int64_t grid_points = 0;
    std::vector<int32_t> points;             // grid points per chromosome of the handle, handle order
    const double *dosage = nullptr;          // device, [n][grid_points][H]; valid until the handle's next grid pass or run
};

// Fills `view` for `sample` (-1: all samples of the run).  make_dosage = false: the shape alone (device, H, n, points),
// no kernel is launched on the handle and `dosage` stays null.  make_dosage = true: the grid kernel runs first under
// gbrs_hmm_match's condition - the handle holds no dosages of the last run for the same `sample` argument - and the call
// returns when the dosages are complete.
int hmm_grid_view(gbrs_hmm *h, int sample, HmmGridView *view, bool make_dosage);

}  // namespace gbrs
