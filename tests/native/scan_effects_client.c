/* A plain C99 client of the founder effects and the LOD support intervals of the genome scan (include/gbrs_hip.h:
 * gbrs_scan_create, _append, _prepare, _effects, _effects_info, _run_support).  tests/test_scan_effects_client.py compiles
 * it with gcc -std=c99 -pedantic -Werror, links it against gbrs_amd/libgbrs_hip.so and compares its output with the numpy
 * restatements of the two rules.
 *
 * Input (little endian): i32 H, i32 n_chrom, i32 n, i32 c, i64 P, i64 T, f64 drop, i32 points[n_chrom] (padded to 8
 *   bytes), i64 column[T], i64 point[T], f64 dosage[n][M][H], f64 qz[n][c], f64 pheno[n][P].
 * Output: f64 effect[T][H], f64 se[T][H], f64 lod[T], f64 sigma2[T], i32 rank[T] (padded to 8 bytes), f64 lod[P][M],
 *   f64 peak_lod[P][n_chrom], i64 peak_index, support_lo, support_hi [P][n_chrom], then a second effect[T][H] and a second
 *   support_lo[P][n_chrom] of refused calls, which must have left the buffers as they were filled.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "gbrs_hip.h"

static void *xread(FILE *f, size_t n) {
    void *p = malloc(n ? n : 1);
    if (!p || fread(p, 1, n, f) != n) {
        fprintf(stderr, "scan_effects_client: short read\n");
        exit(2);
    }
    return p;
}

static void *xalloc(size_t n) {
    void *p = malloc(n ? n : 1);
    if (!p) exit(2);
    return p;
}

#define CHECK(call)                                                              \
    do {                                                                         \
        const int st_ = (call);                                                  \
        if (st_ != GBRS_OK) {                                                    \
            fprintf(stderr, "scan_effects_client: %s -> %d: %s\n", #call, st_, gbrs_last_error()); \
            return 3;                                                            \
        }                                                                        \
    } while (0)

int main(int argc, char **argv) {
    if (argc != 3) return 1;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t head[4];
    int64_t size[2];
    double drop;
    if (fread(head, 4, 4, f) != 4 || fread(size, 8, 2, f) != 2 || fread(&drop, 8, 1, f) != 1) return 2;
    const int H = head[0], n_chrom = head[1], n = head[2], c = head[3];
    const int64_t P = size[0], T = size[1];
    const int32_t *points = (const int32_t *)xread(f, ((size_t)n_chrom * 4 + 7) / 8 * 8);
    int64_t *column = (int64_t *)xread(f, (size_t)T * 8);
    const int64_t *point = (const int64_t *)xread(f, (size_t)T * 8);
    int64_t M = 0, k;
    int ch;
    for (ch = 0; ch < n_chrom; ++ch) M += points[ch];
    const double *dosage = (const double *)xread(f, (size_t)n * M * H * 8);
    const double *qz = (const double *)xread(f, (size_t)n * c * 8);
    const double *pheno = (const double *)xread(f, (size_t)n * P * 8);
    fclose(f);

    const size_t TH = (size_t)(T * H), PC = (size_t)(P * n_chrom), rank_bytes = ((size_t)T * 4 + 7) / 8 * 8;
    gbrs_scan_t *scan = NULL;
    gbrs_scan_effects_info_t info;
    double *effect = (double *)xalloc(TH * 8), *se = (double *)xalloc(TH * 8), *lod = (double *)xalloc((size_t)T * 8);
    double *sigma2 = (double *)xalloc((size_t)T * 8), *refused = (double *)xalloc(TH * 8);
    int32_t *rank = (int32_t *)calloc(rank_bytes, 1);
    double *lods = (double *)xalloc((size_t)(P * M) * 8), *peak_lod = (double *)xalloc(PC * 8);
    int64_t *peak_index = (int64_t *)xalloc(PC * 8), *lo = (int64_t *)xalloc(PC * 8), *hi = (int64_t *)xalloc(PC * 8);
    int64_t *refused_lo = (int64_t *)xalloc(PC * 8);
    if (!rank) return 2;
    for (k = 0; k < (int64_t)TH; ++k) refused[k] = -1.0;
    for (k = 0; k < (int64_t)PC; ++k) refused_lo[k] = -7;
    CHECK(gbrs_scan_create(0, n_chrom, points, H, &scan));
    CHECK(gbrs_scan_append(scan, n, dosage));
    if (gbrs_scan_effects(scan, P, pheno, T, column, point, refused, NULL, NULL, NULL, NULL) != GBRS_ERR_INVALID) return 4;   /* not prepared */
    if (gbrs_scan_run_support(scan, P, pheno, drop, NULL, NULL, NULL, refused_lo, NULL) != GBRS_ERR_INVALID) return 4;
    CHECK(gbrs_scan_prepare(scan, c, qz));
    column[T - 1] += P;                                                           /* a column outside the table */
    if (gbrs_scan_effects(scan, P, pheno, T, column, point, refused, NULL, NULL, NULL, NULL) != GBRS_ERR_INVALID) return 4;
    column[T - 1] -= P;
    if (gbrs_scan_run_support(scan, P, pheno, -1.0, NULL, NULL, NULL, refused_lo, NULL) != GBRS_ERR_INVALID) return 4;
    CHECK(gbrs_scan_effects(scan, P, pheno, T, column, point, effect, se, lod, sigma2, rank));
    CHECK(gbrs_scan_effects_info(scan, &info));
    if (info.T != T || info.P != P || !(info.last_pass_ms > 0.0) || info.peak_device_bytes == 0) return 5;
    printf("scan_effects_client: %lld targets of %lld phenotypes, pass %.3f ms, %llu bytes at the peak\n", (long long)T,
           (long long)P, info.last_pass_ms, (unsigned long long)info.peak_device_bytes);
    CHECK(gbrs_scan_run_support(scan, P, pheno, drop, lods, peak_lod, peak_index, lo, hi));
    f = fopen(argv[2], "wb");
    if (!f) return 2;
    fwrite(effect, 8, TH, f);
    fwrite(se, 8, TH, f);
    fwrite(lod, 8, (size_t)T, f);
    fwrite(sigma2, 8, (size_t)T, f);
    fwrite(rank, 1, rank_bytes, f);
    fwrite(lods, 8, (size_t)(P * M), f);
    fwrite(peak_lod, 8, PC, f);
    fwrite(peak_index, 8, PC, f);
    fwrite(lo, 8, PC, f);
    fwrite(hi, 8, PC, f);
    fwrite(refused, 8, TH, f);
    fwrite(refused_lo, 8, PC, f);
    fclose(f);
    CHECK(gbrs_scan_destroy(scan));
    return 0;
}
