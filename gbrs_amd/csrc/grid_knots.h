// Knots of the grid pass (gbrs_hmm_set_grid): what `gbrs interpolate` hands to interp1d for one chromosome
// (gbrs/gbrs_utils.py:664-688).  Plain C++, no HIP: the same header serves the library and stand-alone host checks.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <numeric>
#include <vector>

namespace gbrs {

// knots = stable sort of [0.0, gene positions..., last grid point + 1.0] (n_genes + 2 of them); knot_gene[k] = the gene
// whose posterior column knot k carries: the knot at 0.0 repeats gene 0, the one past the grid repeats gene n_genes - 1.
// Sorting is what interp1d(assume_sorted=False) does; for the reference's inputs (ascending genes, none beyond the last
// grid point + 1) it is the identity.  Returns 0, or -1 with scipy's ValueError text in `msg` when a grid point lies
// outside the knots, or -2 for arguments that cannot be a grid chromosome.
inline int grid_knots(int n_genes, const double *gene_pos, int n_grid, const double *grid, double *knots,
                      int32_t *knot_gene, char *msg, size_t msg_len) {
    if (n_genes < 1 || n_grid < 1 || !gene_pos || !grid || !knots || !knot_gene) {
        std::snprintf(msg, msg_len, n_genes == 0 ? "index -1 is out of bounds for axis 1 with size 0 (a grid chromosome without genes)"
                                                 : "bad argument");
        return -2;
    }
    const int n = n_genes + 2;
    std::vector<double> x(n);
    x[0] = 0.0;
    std::copy(gene_pos, gene_pos + n_genes, x.begin() + 1);
    x[n - 1] = grid[n_grid - 1] + 1.0;
    std::vector<int32_t> order(n);
    std::iota(order.begin(), order.end(), 0);
    // numpy's order: a NaN (a grid file without a position column) sorts behind every number
    std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) {
        return x[a] < x[b] || (std::isnan(x[b]) && !std::isnan(x[a]));
    });
    for (int k = 0; k < n; ++k) {
        knots[k] = x[order[k]];
        knot_gene[k] = std::min(std::max(order[k] - 1, 0), n_genes - 1);
    }
    for (int g = 0; g < n_grid; ++g) {
        if (grid[g] < knots[0]) {
            std::snprintf(msg, msg_len, "A value (%.17g) in x_new is below the interpolation range's minimum value (%.17g).",
                          grid[g], knots[0]);
            return -1;
        }
        if (grid[g] > knots[n - 1]) {
            std::snprintf(msg, msg_len, "A value (%.17g) in x_new is above the interpolation range's maximum value (%.17g).",
                          grid[g], knots[n - 1]);
            return -1;
        }
    }
    return 0;
}

}  // namespace gbrs
