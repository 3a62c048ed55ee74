// The passes over a finished run of the `gbrs reconstruct` HMM (hmm.hip): grid dosages, panel matching, SNP imputation,
// path draws, diagnostics with pair posteriors, and log-likelihoods, each with its kernels in its own .inc file, and the
// stand-alone interpolation and dosage entry points.  They read what gbrs_hmm_run left on the handle (hmm_handle.h); of
// the core's code they call hmm_make_logs alone.
#include "hmm_handle.h"
#include "grid_knots.h"
#include "scan_hmm.h"

#include <algorithm>
#include <cfloat>
#include <climits>
#include <cmath>
#include <cstdlib>

namespace gbrs {

// ---- post-processing of the posteriors (gbrs_utils.py:612-697 interpolate, :863-938 export) ---

// Linear interpolation of the rows of y (S x n points at ascending x) onto xq, operation order of
// scipy interp1d(kind='linear'):  slope = (y_hi - y_lo) / (x_hi - x_lo);  y = slope * (x - x_lo) + y_lo
__global__ void interpolate_kernel(int S, int n, const double *__restrict__ xs, const double *__restrict__ y,
                                   int m, const double *__restrict__ xq, double *__restrict__ out) {
    const int64_t id = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= (int64_t)S * m) return;
    const int s = (int)(id / m), g = (int)(id - (int64_t)s * m);
    const double x = xq[g];
    int lo = 0, hi = n;                        // searchsorted(xs, x, side='left')
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (xs[mid] < x) lo = mid + 1; else hi = mid;
    }
    const int idx = min(max(lo, 1), n - 1);
    const double x_lo = xs[idx - 1], x_hi = xs[idx];
    const double y_lo = y[(int64_t)s * n + idx - 1], y_hi = y[(int64_t)s * n + idx];
    const double slope = (y_hi - y_lo) / (x_hi - x_lo);
    out[(int64_t)s * m + g] = slope * (x - x_lo) + y_lo;
}

// 36 -> 8 dosage: out[r][h] = sum_g gprob[r][g] * 0.5 * (#h in genotype g)  (convmat, :896-901, :927)
__global__ void dosage_kernel(int H, int S, int64_t rows, const double *__restrict__ gprob,
                              double *__restrict__ out) {
    const int64_t id = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (id >= rows * H) return;
    const int64_t r = id / H;
    const int h = (int)(id - r * H);
    const double *p = gprob + r * S;
    double acc = 0.0;
    int g = 0;
    for (int a = 0; a < H; ++a)
        for (int b = a; b < H; ++b, ++g) {
            const double w = 0.5 * ((a == h) + (b == h));
            acc += p[g] * w;
        }
    out[id] = acc;
}

#include "hmm_grid.inc"
#include "hmm_match.inc"
#include "hmm_impute.inc"
#include "hmm_sample.inc"
#include "hmm_diag.inc"
#include "hmm_loglik.inc"

}  // namespace gbrs

using namespace gbrs;

namespace {

// ---- what the passes do around their kernels ----------------------------------------------------
// The checks are steps, not one call: the passes put their own checks between them, and the first error counts.
int pass_ran(const gbrs_hmm *h) {
    if (!h) return fail(GBRS_ERR_INVALID, "handle is NULL");
    if (!h->ran) return fail(GBRS_ERR_STATE, "run() has not been called");
    return GBRS_OK;
}

// `sample` names one sample of the last run or, as -1, all of them: n samples from sample0 on
int pass_samples(const gbrs_hmm *h, int sample, int *n, int *sample0 = nullptr) {
    if (sample < -1 || sample >= h->n_samples) return fail(GBRS_ERR_INVALID, "sample out of range");
    *n = sample < 0 ? h->n_samples : 1;
    if (sample0) *sample0 = std::max(sample, 0);
    return GBRS_OK;
}

// a buffer that grows to the largest call (those that follow the last call's size are allocated where they are used)
template <typename T>
int ensure(DevBuf<T> &buf, size_t n) { return buf.n < n ? buf.alloc(n) : GBRS_OK; }

// A timed region of the handle's stream opens with a record of ev[0].  This closes it with ev[last] and waits for it.
int timed_wait(gbrs_hmm *h, int last = 1) {
    GBRS_HIP_CHECK(hipEventRecord(h->ev[last], h->stream));
    GBRS_HIP_CHECK(hipGetLastError());
    GBRS_HIP_CHECK(hipStreamSynchronize(h->stream));
    return GBRS_OK;
}

// device milliseconds between two of the handle's events; `unread` (0.0, or the time to keep) where they cannot be read
double elapsed_ms(const gbrs_hmm *h, int from, int to, double unread) {
    float ms = 0.f;
    return hipEventElapsedTime(&ms, h->ev[from], h->ev[to]) == hipSuccess ? ms : unread;
}

// the first `count` elements of a result to the caller, where the caller asked for it
template <typename T>
int copy_out(T *dst, const DevBuf<T> &buf, size_t count) {
    if (dst) GBRS_HIP_CHECK(hipMemcpy(dst, buf.p, count * sizeof(T), hipMemcpyDeviceToHost));
    return GBRS_OK;
}

// the founder-change table of the path draws and of the pair pass, uploaded by the first call that needs it
int ensure_change_table(gbrs_hmm *h) {
    if (h->change_tab.p) return GBRS_OK;
    const std::vector<uint8_t> tab = sample_change_table(h->H);
    GBRS_TRY(h->change_tab.alloc(tab.size()));
    GBRS_HIP_CHECK(hipMemcpy(h->change_tab.p, tab.data(), tab.size(), hipMemcpyHostToDevice));
    return GBRS_OK;
}

void match_clear_panel(gbrs_hmm *h) {
    h->match.panel.release();
    h->match.d_chroms.release();
    h->match.panel_norm.clear();
    h->match.n_panel = 0;
}

}  // namespace

extern "C" {

int gbrs_interpolate(int S, int n_points, const double *x, const double *y, int n_grid,
                     const double *x_grid, double *out, int device) {
    if (S < 1 || n_points < 2 || n_grid < 0 || !x || !y || (n_grid && (!x_grid || !out)))
        return fail(GBRS_ERR_INVALID, "bad argument");
    for (int i = 0; i + 1 < n_points; ++i)
        if (!(x[i] <= x[i + 1])) return fail(GBRS_ERR_INVALID, "x must be ascending");
    for (int g = 0; g < n_grid; ++g) {
        if (x_grid[g] < x[0])
            return fail(GBRS_ERR_INVALID, "A value (%.17g) in x_new is below the interpolation range's minimum value (%.17g).",
                        x_grid[g], x[0]);
        if (x_grid[g] > x[n_points - 1])
            return fail(GBRS_ERR_INVALID, "A value (%.17g) in x_new is above the interpolation range's maximum value (%.17g).",
                        x_grid[g], x[n_points - 1]);
    }
    if (n_grid == 0) return GBRS_OK;
    GBRS_TRY(select_device(device));
    DevBuf<double> d_x, d_y, d_q, d_o;
    GBRS_TRY(d_x.alloc(n_points));
    GBRS_TRY(d_y.alloc((size_t)S * n_points));
    GBRS_TRY(d_q.alloc(n_grid));
    GBRS_TRY(d_o.alloc((size_t)S * n_grid));
    GBRS_HIP_CHECK(hipMemcpy(d_x.p, x, d_x.bytes(), hipMemcpyHostToDevice));
    GBRS_HIP_CHECK(hipMemcpy(d_y.p, y, d_y.bytes(), hipMemcpyHostToDevice));
    GBRS_HIP_CHECK(hipMemcpy(d_q.p, x_grid, d_q.bytes(), hipMemcpyHostToDevice));
    const int64_t total = (int64_t)S * n_grid;
    hipLaunchKernelGGL(interpolate_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, nullptr, S, n_points,
                       d_x.p, d_y.p, n_grid, d_q.p, d_o.p);
    GBRS_HIP_CHECK(hipGetLastError());
    GBRS_HIP_CHECK(hipMemcpy(out, d_o.p, d_o.bytes(), hipMemcpyDeviceToHost));
    return GBRS_OK;
}

int gbrs_genoprob_dosage(int num_haps, int64_t n_rows, const double *gprob, double *out, int device) {
    if (num_haps < 1 || num_haps > MAX_H || n_rows < 0 || (n_rows && (!gprob || !out)))
        return fail(GBRS_ERR_INVALID, "bad argument");
    if (n_rows == 0) return GBRS_OK;
    GBRS_TRY(select_device(device));
    const int S = num_haps * (num_haps + 1) / 2;
    DevBuf<double> d_p, d_o;
    GBRS_TRY(d_p.alloc((size_t)n_rows * S));
    GBRS_TRY(d_o.alloc((size_t)n_rows * num_haps));
    GBRS_HIP_CHECK(hipMemcpy(d_p.p, gprob, d_p.bytes(), hipMemcpyHostToDevice));
    const int64_t total = n_rows * num_haps;
    hipLaunchKernelGGL(dosage_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, nullptr, num_haps, S, n_rows,
                       d_p.p, d_o.p);
    GBRS_HIP_CHECK(hipGetLastError());
    GBRS_HIP_CHECK(hipMemcpy(out, d_o.p, d_o.bytes(), hipMemcpyDeviceToHost));
    return GBRS_OK;
}

int gbrs_grid_knots(int n_genes, const double *gene_pos, int n_grid, const double *grid, double *knots,
                    int32_t *knot_gene) {
    char msg[256];
    if (grid_knots(n_genes, gene_pos, n_grid, grid, knots, knot_gene, msg, sizeof msg) != 0)
        return fail(GBRS_ERR_INVALID, "%s", msg);
    return GBRS_OK;
}

int gbrs_hmm_set_grid(gbrs_hmm_t *h, const int32_t *n_pos, const double *const *gene_pos, const int32_t *n_grid,
                      const double *const *grid) {
    if (!h || !n_pos || !gene_pos || !n_grid || !grid) return fail(GBRS_ERR_INVALID, "bad argument");
    // everything is prepared and checked on the host before the handle changes
    const int P = grid_tile_points(h->S);
    std::vector<GridChrom> gc(h->n_chrom);
    std::vector<GridTile> tiles;
    std::vector<double> knot_x, x;
    std::vector<int32_t> knot_gene;
    for (int c = 0; c < h->n_chrom; ++c) {
        const ChromDesc &cd = h->chroms[c];
        GridChrom &g = gc[c];
        g.gene_off = cd.gene_off;
        g.knot_off = (int32_t)knot_x.size();
        g.point_off = (int32_t)x.size();
        g.n_knots = g.n_points = 0;
        if (n_grid[c] < 0) return fail(GBRS_ERR_INVALID, "n_grid[%d] is negative", c);
        if (n_grid[c] == 0) continue;
        if (n_pos[c] == 0)
            return fail(GBRS_ERR_INVALID, "index -1 is out of bounds for axis 1 with size 0 (grid chromosome %d has no genes)", c);
        if (n_pos[c] != cd.n_genes)
            return fail(GBRS_ERR_INVALID, "chromosome %d: %d gene positions for %d genes", c, n_pos[c], cd.n_genes);
        if ((int64_t)x.size() + n_grid[c] > INT32_MAX) return fail(GBRS_ERR_INVALID, "too many grid points");
        g.n_knots = cd.n_genes + 2;
        g.n_points = n_grid[c];
        knot_x.resize(knot_x.size() + g.n_knots);
        knot_gene.resize(knot_x.size());
        GBRS_TRY(gbrs_grid_knots(cd.n_genes, gene_pos[c], n_grid[c], grid[c], knot_x.data() + g.knot_off,
                                 knot_gene.data() + g.knot_off));
        x.insert(x.end(), grid[c], grid[c] + n_grid[c]);
        for (int32_t first = 0; first < g.n_points; first += P) tiles.push_back(GridTile{c, first});
    }
    GBRS_TRY(select_device(h->device));
    DevBuf<GridChrom> d_gc;
    DevBuf<GridTile> d_tiles;
    DevBuf<double> d_knot_x, d_x;
    DevBuf<int32_t> d_knot_gene;
    GBRS_TRY(d_gc.alloc(gc.size()));
    GBRS_TRY(d_tiles.alloc(tiles.size()));
    GBRS_TRY(d_knot_x.alloc(knot_x.size()));
    GBRS_TRY(d_knot_gene.alloc(knot_gene.size()));
    GBRS_TRY(d_x.alloc(x.size()));
    GBRS_HIP_CHECK(hipMemcpy(d_gc.p, gc.data(), d_gc.bytes(), hipMemcpyHostToDevice));
    if (!tiles.empty()) {
        GBRS_HIP_CHECK(hipMemcpy(d_tiles.p, tiles.data(), d_tiles.bytes(), hipMemcpyHostToDevice));
        GBRS_HIP_CHECK(hipMemcpy(d_knot_x.p, knot_x.data(), d_knot_x.bytes(), hipMemcpyHostToDevice));
        GBRS_HIP_CHECK(hipMemcpy(d_knot_gene.p, knot_gene.data(), d_knot_gene.bytes(), hipMemcpyHostToDevice));
        GBRS_HIP_CHECK(hipMemcpy(d_x.p, x.data(), d_x.bytes(), hipMemcpyHostToDevice));
    }
    h->grid.d_chroms.swap(d_gc);
    h->grid.d_tiles.swap(d_tiles);
    h->grid.knot_x.swap(d_knot_x);
    h->grid.knot_gene.swap(d_knot_gene);
    h->grid.x.swap(d_x);
    h->grid.tiles = (int)tiles.size();
    h->grid.points = (int64_t)x.size();
    h->grid.have = true;
    h->grid.invalidate();               // of another grid
    match_clear_panel(h);
    return GBRS_OK;
}

// What gbrs_hmm_grid and hmm_grid_view check before they touch the device; n: the samples the call is about.
static int hmm_grid_check(const gbrs_hmm *h, int sample, int *n) {
    GBRS_TRY(pass_ran(h));
    if (!h->grid.have) return fail(GBRS_ERR_INVALID, "no grid on the handle: call gbrs_hmm_set_grid first");
    return pass_samples(h, sample, n);
}

// The grid kernel for `sample` (-1: all n) into grid.dosage and / or grid.gamma, timed into grid.ms; returns when it is done.
static int hmm_grid_launch(gbrs_hmm *h, int sample, bool want_dosage, bool want_gamma) {
    const int S = h->S, H = h->H;
    const int n = sample < 0 ? h->n_samples : 1;
    const size_t n_dosage = (size_t)n * h->grid.points * H, n_gamma = (size_t)n * h->grid.points * S;
    if (want_dosage) h->grid.invalidate();
    if (want_dosage && h->grid.dosage.n != n_dosage) GBRS_TRY(h->grid.dosage.alloc(n_dosage));
    if (want_gamma && h->grid.gamma.n != n_gamma) GBRS_TRY(h->grid.gamma.alloc(n_gamma));
    const dim3 grid((unsigned)h->grid.tiles, (unsigned)n);
    const size_t lds = grid_tile_lds(S);
    auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, grid, dim3(64), lds, h->stream, H, S, grid_tile_points(S), h->total_genes, h->grid.points,
                           std::max(sample, 0), h->grid.d_chroms.p, h->grid.d_tiles.p, h->grid.knot_x.p, h->grid.knot_gene.p,
                           h->grid.x.p, h->gamma.p, want_dosage ? h->grid.dosage.p : nullptr, want_gamma ? h->grid.gamma.p : nullptr);
    };
    GBRS_HIP_CHECK(hipEventRecord(h->ev[0], h->stream));
    if (S <= 64) launch(grid_kernel<1>);
    else if (S <= 128) launch(grid_kernel<2>);
    else launch(grid_kernel<3>);          // S <= 136 (MAX_H = 16)
    GBRS_TRY(timed_wait(h));
    h->grid.ms = elapsed_ms(h, 0, 1, h->grid.ms);
    if (want_dosage) {
        h->grid.dosage_ready = true;
        h->grid.dosage_sample = sample;
    }
    return GBRS_OK;
}

int gbrs_hmm_grid(gbrs_hmm_t *h, int sample, double *dosage, double *gamma_grid) {
    RoctxRange roctx_range("gbrs_hmm_grid");
    int n;
    GBRS_TRY(hmm_grid_check(h, sample, &n));
    if ((!dosage && !gamma_grid) || h->grid.tiles == 0) return GBRS_OK;
    GBRS_TRY(select_device(h->device));
    GBRS_TRY(hmm_grid_launch(h, sample, dosage != nullptr, gamma_grid != nullptr));
    GBRS_TRY(copy_out(dosage, h->grid.dosage, (size_t)n * h->grid.points * h->H));
    return copy_out(gamma_grid, h->grid.gamma, (size_t)n * h->grid.points * h->S);
}

int gbrs_hmm_grid_info(gbrs_hmm_t *h, int64_t *n_points, double *last_ms) {
    if (!h) return fail(GBRS_ERR_INVALID, "handle is NULL");
    if (n_points) *n_points = h->grid.have ? h->grid.points : 0;
    if (last_ms) *last_ms = h->grid.ms;
    return GBRS_OK;
}

int gbrs_hmm_set_panel(gbrs_hmm_t *h, int n_panel, const double *const *panel) {
    RoctxRange roctx_range("gbrs_hmm_set_panel");
    if (!h) return fail(GBRS_ERR_INVALID, "handle is NULL");
    if (n_panel < 0 || (n_panel > 0 && !panel)) return fail(GBRS_ERR_INVALID, "bad argument");
    if (!h->grid.have) return fail(GBRS_ERR_INVALID, "no grid on the handle: call gbrs_hmm_set_grid first");
    if (n_panel == 0) {
        match_clear_panel(h);
        return GBRS_OK;
    }
    // everything is prepared and checked before the handle changes
    const int64_t ld = h->grid.points * h->H;
    for (int j = 0; j < n_panel; ++j) {
        if (!panel[j]) return fail(GBRS_ERR_INVALID, "panel[%d] is NULL", j);
        for (int64_t k = 0; k < ld; ++k)
            if (!std::isfinite(panel[j][k]))
                return fail(GBRS_ERR_INVALID, "panel entry %d holds a value that is not finite (grid point %lld, founder %d)", j,
                            (long long)(k / h->H), (int)(k % h->H));
    }
    std::vector<GridChrom> gc(h->n_chrom);
    std::vector<MatchChrom> mc;
    GBRS_TRY(select_device(h->device));
    GBRS_HIP_CHECK(hipMemcpy(gc.data(), h->grid.d_chroms.p, gc.size() * sizeof(GridChrom), hipMemcpyDeviceToHost));
    for (int c = 0; c < h->n_chrom; ++c)
        if (gc[c].n_points > 0)
            mc.push_back(MatchChrom{(int64_t)gc[c].point_off * h->H, (int64_t)gc[c].n_points * h->H, c});
    DevBuf<double> d_panel, d_norm;
    DevBuf<MatchChrom> d_mc;
    GBRS_TRY(d_panel.alloc((size_t)n_panel * ld));
    GBRS_TRY(d_norm.alloc((size_t)n_panel * h->n_chrom));
    GBRS_TRY(d_mc.alloc(mc.size()));
    std::vector<double> norm((size_t)n_panel * h->n_chrom, 0.0);
    if (ld > 0) {
        for (int j = 0; j < n_panel; ++j)
            GBRS_HIP_CHECK(hipMemcpy(d_panel.p + (size_t)j * ld, panel[j], (size_t)ld * sizeof(double), hipMemcpyHostToDevice));
        GBRS_HIP_CHECK(hipMemcpy(d_mc.p, mc.data(), d_mc.bytes(), hipMemcpyHostToDevice));
        hipLaunchKernelGGL(match_norm_kernel, dim3((unsigned)n_panel, (unsigned)h->n_chrom), dim3(64), 0, h->stream, h->H, ld,
                           h->grid.d_chroms.p, d_panel.p, d_norm.p);
        GBRS_HIP_CHECK(hipGetLastError());
        GBRS_HIP_CHECK(hipStreamSynchronize(h->stream));
        GBRS_HIP_CHECK(hipMemcpy(norm.data(), d_norm.p, d_norm.bytes(), hipMemcpyDeviceToHost));
    }
    h->match.panel.swap(d_panel);
    h->match.d_chroms.swap(d_mc);
    h->match.panel_norm.swap(norm);
    h->match.n_panel = n_panel;
    h->match.vec2 = h->H % 2 == 0;           // ld and every chromosome's first column are multiples of H
    return GBRS_OK;
}

int gbrs_hmm_match(gbrs_hmm_t *h, int sample, double *cross, double *sample_norm) {
    RoctxRange roctx_range("gbrs_hmm_match");
    int n;
    GBRS_TRY(pass_ran(h));
    if (!h->grid.have || h->match.n_panel == 0) return fail(GBRS_ERR_INVALID, "no panel on the handle: call gbrs_hmm_set_panel first");
    GBRS_TRY(pass_samples(h, sample, &n));
    GBRS_TRY(select_device(h->device));
    const int M = h->match.n_panel, n_chrom = h->n_chrom;
    const int64_t ld = h->grid.points * h->H;
    const size_t n_cross = (size_t)n * n_chrom * M, n_norm = (size_t)n * n_chrom;
    if (h->match.cross.n != n_cross) GBRS_TRY(h->match.cross.alloc(n_cross));      // (device_bytes: the last call's)
    if (h->match.snorm.n != n_norm) GBRS_TRY(h->match.snorm.alloc(n_norm));
    const unsigned on_grid = (unsigned)h->match.d_chroms.n;
    if (on_grid && !(h->grid.dosage_ready && h->grid.dosage_sample == sample))
        GBRS_TRY(hmm_grid_launch(h, sample, true, false));
    GBRS_HIP_CHECK(hipEventRecord(h->ev[0], h->stream));
    GBRS_HIP_CHECK(hipMemsetAsync(h->match.cross.p, 0, h->match.cross.bytes(), h->stream));    // chromosomes off the grid: 0.0
    GBRS_HIP_CHECK(hipMemsetAsync(h->match.snorm.p, 0, h->match.snorm.bytes(), h->stream));
    if (on_grid) {
        hipLaunchKernelGGL(match_norm_kernel, dim3((unsigned)n, (unsigned)n_chrom), dim3(64), 0, h->stream, h->H, ld,
                           h->grid.d_chroms.p, h->grid.dosage.p, h->match.snorm.p);
        const dim3 grid((unsigned)((n + MT_ROWS - 1) / MT_ROWS), (unsigned)((M + MT_COLS - 1) / MT_COLS), on_grid);
        auto launch = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, grid, dim3(MT_THREADS), 0, h->stream, n, M, n_chrom, ld, h->match.d_chroms.p,
                               h->grid.dosage.p, h->match.panel.p, h->match.cross.p);
        };
        if (h->match.vec2) launch(match_cross_kernel<true>);
        else launch(match_cross_kernel<false>);
    }
    GBRS_TRY(timed_wait(h));
    h->match.ms = elapsed_ms(h, 0, 1, h->match.ms);
    GBRS_TRY(copy_out(cross, h->match.cross, n_cross));
    return copy_out(sample_norm, h->match.snorm, n_norm);
}

int gbrs_hmm_match_info(gbrs_hmm_t *h, int *n_panel, double *panel_norm, double *last_ms, uint64_t *device_bytes) {
    if (!h) return fail(GBRS_ERR_INVALID, "handle is NULL");
    if (n_panel) *n_panel = h->match.n_panel;
    if (panel_norm && !h->match.panel_norm.empty()) std::memcpy(panel_norm, h->match.panel_norm.data(), h->match.panel_norm.size() * sizeof(double));
    if (last_ms) *last_ms = h->match.ms;
    if (device_bytes)
        *device_bytes = h->match.panel.bytes() + h->match.cross.bytes() + h->match.snorm.bytes() + h->match.d_chroms.bytes();
    return GBRS_OK;
}

int gbrs_hmm_set_snps(gbrs_hmm_t *h, const int32_t *n_pos, const double *const *gene_pos, const int32_t *n_snps,
                      const double *const *snp_pos, const uint32_t *const *snp_mask) {
    RoctxRange roctx_range("gbrs_hmm_set_snps");
    if (!h || !n_pos || !gene_pos || !n_snps || !snp_pos || !snp_mask) return fail(GBRS_ERR_INVALID, "bad argument");
    // everything is prepared and checked before the handle changes
    std::vector<SnpChrom> sc(h->n_chrom);
    std::vector<double> knot_x;
    std::vector<int32_t> knot_gene, knot_row;
    int64_t total = 0;
    const uint32_t beyond = h->H >= 32 ? 0u : ~0u << h->H;
    if (h->total_genes + 2 * (int64_t)h->n_chrom > INT32_MAX) return fail(GBRS_ERR_INVALID, "too many genes for SNP knots");
    for (int c = 0; c < h->n_chrom; ++c) {
        const ChromDesc &cd = h->chroms[c];
        SnpChrom &s = sc[c];
        s.gene_off = cd.gene_off;
        s.knot_off = (int32_t)knot_x.size();
        s.n_knots = 0;
        s.snp_off = total;
        if (n_snps[c] < 0) return fail(GBRS_ERR_INVALID, "n_snps[%d] is negative", c);
        if (n_snps[c] == 0) continue;
        if (!snp_pos[c] || !snp_mask[c]) return fail(GBRS_ERR_INVALID, "chromosome %d: SNP positions or patterns are NULL", c);
        if (n_pos[c] == 0)
            return fail(GBRS_ERR_INVALID, "index -1 is out of bounds for axis 1 with size 0 (SNP chromosome %d has no genes)", c);
        if (n_pos[c] != cd.n_genes)
            return fail(GBRS_ERR_INVALID, "chromosome %d: %d gene positions for %d genes", c, n_pos[c], cd.n_genes);
        for (int32_t k = 0; k < n_snps[c]; ++k)
            if (snp_mask[c][k] & beyond)
                return fail(GBRS_ERR_INVALID, "chromosome %d, SNP %d: the pattern 0x%x names a founder at or above %d", c, k,
                            snp_mask[c][k], h->H);
        s.n_knots = cd.n_genes + 2;
        knot_x.resize(knot_x.size() + s.n_knots);
        knot_gene.resize(knot_x.size());
        GBRS_TRY(gbrs_grid_knots(cd.n_genes, gene_pos[c], n_snps[c], snp_pos[c], knot_x.data() + s.knot_off,
                                 knot_gene.data() + s.knot_off));
        total += n_snps[c];
    }
    if (total == 0) {
        h->snp.d_chroms.release();
        h->snp.knot_x.release();
        h->snp.knot_row.release();
        h->snp.x.release();
        h->snp.mask.release();
        h->snp.idx.release();
        h->snp.out.release();
        h->snp.n = 0;
        return GBRS_OK;
    }
    knot_row.resize(knot_gene.size());
    for (int c = 0; c < h->n_chrom; ++c)
        for (int32_t k = 0; k < sc[c].n_knots; ++k)
            knot_row[sc[c].knot_off + k] = (int32_t)(sc[c].gene_off + knot_gene[sc[c].knot_off + k]);
    GBRS_TRY(select_device(h->device));
    DevBuf<SnpChrom> d_sc;
    DevBuf<double> d_knot_x, d_x;
    DevBuf<int32_t> d_knot_row, d_idx;
    DevBuf<uint32_t> d_mask;
    GBRS_TRY(d_sc.alloc(sc.size()));
    GBRS_TRY(d_knot_x.alloc(knot_x.size()));
    GBRS_TRY(d_knot_row.alloc(knot_row.size()));
    GBRS_TRY(d_x.alloc((size_t)total));
    GBRS_TRY(d_mask.alloc((size_t)total));
    GBRS_TRY(d_idx.alloc((size_t)total));
    GBRS_HIP_CHECK(hipMemcpy(d_sc.p, sc.data(), d_sc.bytes(), hipMemcpyHostToDevice));
    GBRS_HIP_CHECK(hipMemcpy(d_knot_x.p, knot_x.data(), d_knot_x.bytes(), hipMemcpyHostToDevice));
    GBRS_HIP_CHECK(hipMemcpy(d_knot_row.p, knot_row.data(), d_knot_row.bytes(), hipMemcpyHostToDevice));
    for (int c = 0; c < h->n_chrom; ++c) {
        if (n_snps[c] == 0) continue;
        GBRS_HIP_CHECK(hipMemcpy(d_x.p + sc[c].snp_off, snp_pos[c], (size_t)n_snps[c] * sizeof(double), hipMemcpyHostToDevice));
        GBRS_HIP_CHECK(hipMemcpy(d_mask.p + sc[c].snp_off, snp_mask[c], (size_t)n_snps[c] * sizeof(uint32_t),
                                 hipMemcpyHostToDevice));
    }
    GBRS_HIP_CHECK(hipEventRecord(h->ev[0], h->stream));
    hipLaunchKernelGGL(snp_setup_kernel, dim3((unsigned)((total + IMPUTE_THREADS - 1) / IMPUTE_THREADS)), dim3(IMPUTE_THREADS), 0,
                       h->stream, h->n_chrom, total, d_sc.p, d_knot_x.p, d_x.p, d_idx.p);
    GBRS_TRY(timed_wait(h));
    h->snp.ms_setup = elapsed_ms(h, 0, 1, 0.0);
    h->snp.d_chroms.swap(d_sc);
    h->snp.knot_x.swap(d_knot_x);
    h->snp.knot_row.swap(d_knot_row);
    h->snp.x.swap(d_x);
    h->snp.mask.swap(d_mask);
    h->snp.idx.swap(d_idx);
    h->snp.n = total;
    return GBRS_OK;
}

int gbrs_hmm_impute(gbrs_hmm_t *h, int sample, int64_t first, int64_t count, double *out) {
    RoctxRange roctx_range("gbrs_hmm_impute");
    int n, sample0;
    GBRS_TRY(pass_ran(h));
    if (h->snp.n == 0) return fail(GBRS_ERR_INVALID, "no SNPs on the handle: call gbrs_hmm_set_snps first");
    GBRS_TRY(pass_samples(h, sample, &n, &sample0));
    if (first < 0 || count < 0 || first > h->snp.n || count > h->snp.n - first)
        return fail(GBRS_ERR_INVALID, "SNPs %lld .. %lld are outside 0 .. %lld", (long long)first, (long long)first + count,
                    (long long)h->snp.n);
    if (count == 0) return GBRS_OK;
    if (!out) return fail(GBRS_ERR_INVALID, "out is NULL");
    GBRS_TRY(select_device(h->device));
    const int S = h->S, H = h->H;
    const size_t n_out = (size_t)n * count;
    GBRS_TRY(ensure(h->snp.out, n_out));
    const bool make_d = !(h->snp.d_ready && h->snp.d_sample == sample);
    GBRS_HIP_CHECK(hipEventRecord(h->ev[0], h->stream));
    if (make_d) {
        const int64_t rows = (int64_t)n * h->total_genes;
        h->snp.invalidate();
        if (h->snp.d.n != (size_t)rows * H) GBRS_TRY(h->snp.d.alloc((size_t)rows * H));      // (device_bytes: the last pass's)
        hipLaunchKernelGGL(dosage_kernel, dim3((unsigned)((rows * H + 255) / 256)), dim3(256), 0, h->stream, H, S, rows,
                           h->gamma.p + (int64_t)sample0 * h->total_genes * S, h->snp.d.p);
    }
    GBRS_HIP_CHECK(hipEventRecord(h->ev[1], h->stream));
    const dim3 grid((unsigned)((count + IMPUTE_THREADS - 1) / IMPUTE_THREADS), (unsigned)((n + IMPUTE_SAMPLES - 1) / IMPUTE_SAMPLES));
    auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, grid, dim3(IMPUTE_THREADS), 0, h->stream, H, n, h->total_genes, first, count, h->snp.knot_x.p,
                           h->snp.knot_row.p, h->snp.x.p, h->snp.mask.p, h->snp.idx.p, h->snp.d.p, h->snp.out.p);
    };
    if (H == 8) launch(impute_kernel<true, 8>);
    else if (H % 2 == 0) launch(impute_kernel<true, 0>);
    else launch(impute_kernel<false, 0>);
    GBRS_TRY(timed_wait(h, 2));
    h->snp.ms_d = make_d ? elapsed_ms(h, 0, 1, 0.0) : 0.0;
    h->snp.ms_kernel = elapsed_ms(h, 1, 2, 0.0);
    h->snp.d_ready = true;
    h->snp.d_sample = sample;
    return copy_out(out, h->snp.out, n_out);
}

int gbrs_hmm_impute_info(gbrs_hmm_t *h, int64_t *n_snps, double *last_ms, uint64_t *device_bytes) {
    if (!h) return fail(GBRS_ERR_INVALID, "handle is NULL");
    if (n_snps) *n_snps = h->snp.n;
    if (last_ms) *last_ms = h->snp.ms_d + h->snp.ms_kernel;
    if (device_bytes)
        *device_bytes = h->snp.d_chroms.bytes() + h->snp.knot_x.bytes() + h->snp.knot_row.bytes() + h->snp.x.bytes() +
                        h->snp.mask.bytes() + h->snp.idx.bytes() + h->snp.d.bytes() + h->snp.out.bytes();
    return GBRS_OK;
}

int gbrs_hmm_impute_times(gbrs_hmm_t *h, double *setup_ms, double *dosage_ms, double *kernel_ms) {
    if (!h) return fail(GBRS_ERR_INVALID, "handle is NULL");
    if (setup_ms) *setup_ms = h->snp.ms_setup;
    if (dosage_ms) *dosage_ms = h->snp.ms_d;
    if (kernel_ms) *kernel_ms = h->snp.ms_kernel;
    return GBRS_OK;
}

int gbrs_hmm_sample_paths(gbrs_hmm_t *h, int sample, int n_draws, uint64_t seed, const uint32_t *streams, uint8_t *paths,
                          int32_t *changes, uint64_t *degenerate) {
    RoctxRange roctx_range("gbrs_hmm_sample_paths");
    int n, sample0;
    GBRS_TRY(pass_ran(h));
    if (n_draws < 1) return fail(GBRS_ERR_INVALID, "n_draws must be at least 1");
    GBRS_TRY(pass_samples(h, sample, &n, &sample0));
    if (!paths) return fail(GBRS_ERR_INVALID, "paths is NULL");
    GBRS_TRY(select_device(h->device));
    GBRS_TRY(hmm_make_logs(h));
    const int S = h->S;
    const size_t G = (size_t)h->total_genes;
    // draws per slab: two byte images of n x slab x G (gene-major as drawn, draw-major as returned) within 1 GiB, whole
    // workgroups of draws where that many fit; GBRS_TUNING_SAMPLE_SLAB names a count instead.  The draws are keyed by their
    // number, so the cut changes no value.
    size_t slab = std::max<size_t>(((size_t)1 << 30) / (2 * (size_t)n * G), 1);
    if (slab >= SAMPLE_BLOCK) slab -= slab % SAMPLE_BLOCK;
    if (const char *e = std::getenv("GBRS_TUNING_SAMPLE_SLAB"); e && std::atoi(e) > 0) slab = (size_t)std::atoi(e);
    slab = std::min<size_t>(slab, (size_t)n_draws);
    GBRS_TRY(ensure_change_table(h));
    GBRS_TRY(ensure(h->draws.cols, (size_t)n * slab * G));
    GBRS_TRY(ensure(h->draws.paths, (size_t)n * slab * G));
    if (changes) GBRS_TRY(ensure(h->draws.changes, (size_t)n * slab * h->n_chrom));
    GBRS_TRY(ensure(h->draws.streams, (size_t)n));
    GBRS_TRY(ensure(h->draws.degenerate, 1));
    std::vector<uint32_t> ids((size_t)n);
    for (int k = 0; k < n; ++k) ids[k] = streams ? streams[k] : (uint32_t)(sample0 + k);
    GBRS_HIP_CHECK(hipMemcpy(h->draws.streams.p, ids.data(), ids.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    GBRS_HIP_CHECK(hipMemsetAsync(h->draws.degenerate.p, 0, sizeof(unsigned long long), h->stream));
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    const size_t lds = sample_lds(S);
    h->draws.ms = 0;
    for (size_t d0 = 0; d0 < (size_t)n_draws; d0 += slab) {
        const int ks = (int)std::min<size_t>(slab, (size_t)n_draws - d0);
        const dim3 grid((unsigned)((ks + SAMPLE_BLOCK - 1) / SAMPLE_BLOCK), (unsigned)h->n_chrom, (unsigned)n);
        auto launch = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, grid, dim3(SAMPLE_BLOCK), lds, h->stream, S, h->n_chrom, h->total_genes, sample0,
                               (uint32_t)d0, ks, h->d_chroms.p, h->d_order.p, h->alpha.p, h->tprob.p, h->change_tab.p,
                               h->draws.streams.p, k0, k1, h->draws.cols.p, changes ? h->draws.changes.p : nullptr,
                               h->draws.degenerate.p);
        };
        GBRS_HIP_CHECK(hipEventRecord(h->ev[0], h->stream));
        if (sample_table_in_lds(S)) launch(sample_paths_kernel<true>);
        else launch(sample_paths_kernel<false>);
        hipLaunchKernelGGL(sample_transpose_kernel, dim3((unsigned)((G + 63) / 64), (unsigned)((ks + 63) / 64), (unsigned)n),
                           dim3(256), 0, h->stream, h->total_genes, ks, h->draws.cols.p, h->draws.paths.p);
        GBRS_TRY(timed_wait(h));
        h->draws.ms += elapsed_ms(h, 0, 1, 0.0);            // the slabs' kernels, without the copies between them
        for (int k = 0; k < n; ++k) {       // a sample's draws of this slab are contiguous on both sides
            GBRS_HIP_CHECK(hipMemcpy(paths + ((size_t)k * n_draws + d0) * G, h->draws.paths.p + (size_t)k * ks * G,
                                     (size_t)ks * G, hipMemcpyDeviceToHost));
            if (changes)
                GBRS_HIP_CHECK(hipMemcpy(changes + ((size_t)k * n_draws + d0) * h->n_chrom,
                                         h->draws.changes.p + (size_t)k * ks * h->n_chrom,
                                         (size_t)ks * h->n_chrom * sizeof(int32_t), hipMemcpyDeviceToHost));
        }
    }
    if (degenerate) {
        unsigned long long count = 0;
        GBRS_HIP_CHECK(hipMemcpy(&count, h->draws.degenerate.p, sizeof(count), hipMemcpyDeviceToHost));
        *degenerate = count;
    }
    return GBRS_OK;
}

int gbrs_hmm_sample_info(gbrs_hmm_t *h, double *last_ms, uint64_t *device_bytes) {
    if (!h) return fail(GBRS_ERR_INVALID, "handle is NULL");
    if (last_ms) *last_ms = h->draws.ms;
    if (device_bytes)
        *device_bytes = h->change_tab.bytes() + h->draws.cols.bytes() + h->draws.paths.bytes() + h->draws.changes.bytes() +
                        h->draws.streams.bytes() + h->draws.degenerate.bytes();
    return GBRS_OK;
}

int gbrs_hmm_diagnostics(gbrs_hmm_t *h, int sample, double *xo, double *pswitch, double *errlod, double *maxprob,
                         int32_t *maxmarg) {
    RoctxRange roctx_range("gbrs_hmm_diagnostics");
    int n, sample0;
    GBRS_TRY(pass_ran(h));
    GBRS_TRY(pass_samples(h, sample, &n, &sample0));
    GBRS_TRY(select_device(h->device));
    const int S = h->S;
    const size_t G = (size_t)h->total_genes, cells = (size_t)n * G;
    const bool pair = xo || pswitch, gene = errlod || maxprob || maxmarg;
    h->diag.ms = 0;
    if (cells == 0 || !(pair || gene)) return GBRS_OK;
    if (pair || errlod) GBRS_TRY(hmm_make_logs(h));
    if (pair) GBRS_TRY(ensure_change_table(h));
    if (xo) GBRS_TRY(ensure(h->diag.xo, cells));
    if (pswitch) GBRS_TRY(ensure(h->diag.pswitch, cells));
    if (errlod) GBRS_TRY(ensure(h->diag.errlod, cells));
    if (maxprob) GBRS_TRY(ensure(h->diag.maxprob, cells));
    if (maxmarg) GBRS_TRY(ensure(h->diag.maxmarg, cells));
    GBRS_HIP_CHECK(hipEventRecord(h->ev[0], h->stream));
    if (pair) {
        // samples of one workgroup: it reads a table block once for all of them.  Four per wavefront keep the grid wide
        // at cohort sizes; GBRS_TUNING_DIAG_SLAB names a count instead.  A value does not depend on the cut.
        int slab = 4 * DIAG_WAVES;
        if (const char *e = std::getenv("GBRS_TUNING_DIAG_SLAB"); e && std::atoi(e) > 0) slab = std::atoi(e);
        slab = std::min(slab, n);
        const dim3 grid((unsigned)((G + DIAG_RUN - 1) / DIAG_RUN), (unsigned)((n + slab - 1) / slab));
        auto launch = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, grid, dim3(DIAG_BLOCK), diag_pair_lds(S), h->stream, S, h->n_chrom, h->total_genes,
                               (int64_t)0, h->total_genes, sample0, n, slab, h->d_chroms.p, h->alpha.p, h->beta.p, h->eprob.p,
                               h->tprob.p, h->change_tab.p, xo ? h->diag.xo.p : nullptr,
                               pswitch ? h->diag.pswitch.p : nullptr, (double *)nullptr);
        };
        if (diag_table_in_lds(S)) launch(diag_pair_kernel<true, false>);
        else launch(diag_pair_kernel<false, false>);
    }
    if (gene) {
        const int64_t rows = (int64_t)cells;
        hipLaunchKernelGGL(diag_gene_kernel, dim3((unsigned)((rows + DIAG_WAVES - 1) / DIAG_WAVES)), dim3(DIAG_BLOCK), 0,
                           h->stream, S, h->total_genes, sample0, rows, h->init_vec.p, h->alpha.p, h->beta.p, h->eprob.p,
                           h->gamma.p, errlod ? h->diag.errlod.p : nullptr, maxprob ? h->diag.maxprob.p : nullptr,
                           maxmarg ? h->diag.maxmarg.p : nullptr);
    }
    GBRS_TRY(timed_wait(h));
    h->diag.ms = elapsed_ms(h, 0, 1, h->diag.ms);
    GBRS_TRY(copy_out(xo, h->diag.xo, cells));
    GBRS_TRY(copy_out(pswitch, h->diag.pswitch, cells));
    GBRS_TRY(copy_out(errlod, h->diag.errlod, cells));
    GBRS_TRY(copy_out(maxprob, h->diag.maxprob, cells));
    return copy_out(maxmarg, h->diag.maxmarg, cells);
}

int gbrs_hmm_pair_posterior(gbrs_hmm_t *h, int sample, int chrom, double *xi) {
    RoctxRange roctx_range("gbrs_hmm_pair_posterior");
    GBRS_TRY(pass_ran(h));
    if (sample < 0 || sample >= h->n_samples || chrom < 0 || chrom >= h->n_chrom)
        return fail(GBRS_ERR_INVALID, "sample/chromosome out of range");
    if (!xi) return fail(GBRS_ERR_INVALID, "xi is NULL");
    const ChromDesc &cd = h->chroms[chrom];
    if (cd.n_genes < 2) return GBRS_OK;                  // no interval
    GBRS_TRY(select_device(h->device));
    GBRS_TRY(hmm_make_logs(h));
    GBRS_TRY(ensure_change_table(h));
    const int S = h->S;
    const size_t cells = (size_t)(cd.n_genes - 1) * S * S;
    GBRS_TRY(ensure(h->diag.xi, cells));
    const dim3 grid((unsigned)((cd.n_genes + DIAG_RUN - 1) / DIAG_RUN), 1u);
    auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, grid, dim3(DIAG_BLOCK), diag_pair_lds(S), h->stream, S, h->n_chrom, h->total_genes,
                           cd.gene_off, cd.gene_off + cd.n_genes, sample, 1, 1, h->d_chroms.p, h->alpha.p, h->beta.p,
                           h->eprob.p, h->tprob.p, h->change_tab.p, (double *)nullptr, (double *)nullptr, h->diag.xi.p);
    };
    if (diag_table_in_lds(S)) launch(diag_pair_kernel<true, true>);
    else launch(diag_pair_kernel<false, true>);
    GBRS_HIP_CHECK(hipGetLastError());                   // (not timed)
    GBRS_HIP_CHECK(hipStreamSynchronize(h->stream));
    return copy_out(xi, h->diag.xi, cells);
}

int gbrs_hmm_diagnostics_info(gbrs_hmm_t *h, double *last_ms) {
    if (!h) return fail(GBRS_ERR_INVALID, "handle is NULL");
    if (last_ms) *last_ms = h->diag.ms;
    return GBRS_OK;
}

int gbrs_hmm_loglik(gbrs_hmm_t *h, int sample, double *loglik) {
    RoctxRange roctx_range("gbrs_hmm_loglik");
    int n, sample0;
    GBRS_TRY(pass_ran(h));
    GBRS_TRY(pass_samples(h, sample, &n, &sample0));
    if (!loglik) return fail(GBRS_ERR_INVALID, "loglik is NULL");
    if (h->last.chain_interleaved) return fail(GBRS_ERR_UNSUPPORTED, "the last run left its rows as [gene][sample]");
    GBRS_TRY(select_device(h->device));
    const size_t cells = (size_t)n * h->n_chrom;
    GBRS_TRY(ensure(h->ll.out, cells));
    GBRS_HIP_CHECK(hipEventRecord(h->ev[0], h->stream));
    hipLaunchKernelGGL(loglik_reduce_kernel, dim3((unsigned)((h->n_chrom + LL_RED_WAVES - 1) / LL_RED_WAVES), (unsigned)n),
                       dim3(64 * LL_RED_WAVES), 0, h->stream, h->n_chrom, h->total_genes, sample0, h->d_chroms.p, h->invz.p,
                       h->ll.out.p);
    GBRS_TRY(timed_wait(h));
    h->ll.ms = elapsed_ms(h, 0, 1, 0.0);
    return copy_out(loglik, h->ll.out, cells);
}

int gbrs_hmm_loglik_tables(gbrs_hmm_t *h, int chrom, int n_tables, const int32_t *n_trans, const double *const *tprob,
                           int sample, double *loglik) {
    RoctxRange roctx_range("gbrs_hmm_loglik_tables");
    GBRS_TRY(pass_ran(h));
    if (sample < -1 || sample >= h->n_samples || chrom < 0 || chrom >= h->n_chrom)
        return fail(GBRS_ERR_INVALID, "sample/chromosome out of range");
    if (n_tables < 1) return fail(GBRS_ERR_INVALID, "n_tables must be at least 1");
    if (!n_trans || !tprob || !loglik) return fail(GBRS_ERR_INVALID, "NULL argument");
    const ChromDesc &cd = h->chroms[chrom];
    const int n_steps = cd.n_genes - 1;                    // only T[0 .. n_c - 2] are read
    for (int k = 0; k < n_tables; ++k) {
        if (n_trans[k] < n_steps)
            return fail(GBRS_ERR_INVALID, "index %d is out of bounds for axis 0 with size %d (table %d)", n_steps - 1,
                        n_trans[k], k);
        if (n_steps > 0 && !tprob[k]) return fail(GBRS_ERR_INVALID, "tprob[%d] is NULL", k);
    }
    if (h->last.chain_interleaved) return fail(GBRS_ERR_UNSUPPORTED, "the last run left its rows as [gene][sample]");
    GBRS_TRY(select_device(h->device));
    const int S = h->S, n = sample < 0 ? h->n_samples : 1, sample0 = std::max(sample, 0);
    const size_t per_table = (size_t)n_steps * S * S, cells = (size_t)n_tables * n;
    GBRS_TRY(ensure(h->ll.out, cells));
    if (per_table > 0) {
        GBRS_TRY(ensure(h->ll.t, per_table * n_tables));
        GBRS_TRY(ensure(h->ll.pt, per_table * n_tables));
        for (int k = 0; k < n_tables; ++k)
            GBRS_HIP_CHECK(hipMemcpy(h->ll.t.p + per_table * k, tprob[k], per_table * sizeof(double), hipMemcpyHostToDevice));
    }
    GBRS_HIP_CHECK(hipEventRecord(h->ev[0], h->stream));
    if (per_table > 0)          // P = exp(T) once per candidate table, for every sample of the call
        hipLaunchKernelGGL(exp_blocks_t_kernel, dim3(2048), dim3(256), 0, h->stream, S, (int64_t)n_steps * n_tables, h->ll.t.p,
                           h->ll.pt.p, S == 36);
    auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3((unsigned)cells), dim3(64), 0, h->stream, S, cd.n_genes, cd.gene_off, h->total_genes,
                           sample0, n, (int)cells, h->ll.pt.p, h->peprob.p, h->init_vec.p, h->ll.out.p);
    };
    if (S <= 8) launch(loglik_tables_kernel<1, 8, 3>);
    else if (S <= 16) launch(loglik_tables_kernel<1, 16, 3>);
    else if (S == 36) launch(loglik_tables_kernel<1, 36, 4, 36>);   // 8 founders: the paired layout
    else if (S < 36) launch(loglik_tables_kernel<1, 36, 3>);
    else if (S <= 64) launch(loglik_tables_kernel<1, 64, 2>);
    else launch(loglik_tables_kernel<3, 0, 1>);            // S <= 136 (MAX_H = 16)
    GBRS_TRY(timed_wait(h));
    h->ll.ms = elapsed_ms(h, 0, 1, 0.0);
    return copy_out(loglik, h->ll.out, cells);
}

int gbrs_hmm_loglik_info(gbrs_hmm_t *h, double *last_ms, uint64_t *device_bytes) {
    if (!h) return fail(GBRS_ERR_INVALID, "handle is NULL");
    if (last_ms) *last_ms = h->ll.ms;
    if (device_bytes) *device_bytes = h->ll.out.bytes() + h->ll.t.bytes() + h->ll.pt.bytes();
    return GBRS_OK;
}

}  // extern "C"

// gbrs_warm_up (common.hip): loads this file's code object
namespace gbrs {
__global__ void warm_hmm_passes_kernel() {}
void warm_hmm_passes(hipStream_t st) { hipLaunchKernelGGL(warm_hmm_passes_kernel, dim3(1), dim3(64), 0, st); }
}  // namespace gbrs

// The genome scan's read-only view of the grid dosages (scan_hmm.h).
int gbrs::hmm_grid_view(gbrs_hmm *h, int sample, HmmGridView *view, bool make_dosage) {
    int n;
    if (!h) return fail(GBRS_ERR_INVALID, "hmm handle is NULL");
    GBRS_TRY(hmm_grid_check(h, sample, &n));
    GBRS_TRY(select_device(h->device));
    std::vector<GridChrom> gc(h->n_chrom);
    GBRS_HIP_CHECK(hipMemcpy(gc.data(), h->grid.d_chroms.p, gc.size() * sizeof(GridChrom), hipMemcpyDeviceToHost));
    if (make_dosage && h->grid.tiles > 0 && !(h->grid.dosage_ready && h->grid.dosage_sample == sample))
        GBRS_TRY(hmm_grid_launch(h, sample, true, false));
    view->device = h->device;
    view->H = h->H;
    view->n = n;
    view->grid_points = h->grid.points;
    view->points.resize(h->n_chrom);
    for (int c = 0; c < h->n_chrom; ++c) view->points[c] = gc[c].n_points;
    view->dosage = make_dosage ? h->grid.dosage.p : nullptr;
    return GBRS_OK;
}
