/* A plain C99 client of the founder effects and support intervals under the mixed model (include/gbrs_hip.h:
 * gbrs_scan_lmm_effects, gbrs_scan_lmm_effects_info, gbrs_scan_lmm_run_support).  tests/test_scan_lmm_effects_client.py
 * compiles it with gcc -std=c99 -pedantic -Werror, links it against gbrs_amd/libgbrs_hip.so and compares its output with
 * the numpy restatements.  The client brings its own decompositions: it reads them from the fixture the test writes.
 *
 * Input (little endian): i32 H, i32 n_chrom, i32 n, i32 cz, i32 n_eig, i32 reserved, i64 P, i64 T, f64 drop,
 *   i32 points[n_chrom] (padded to 8 bytes), i32 eig_of_chrom[n_chrom] (padded to 8 bytes), f64 dosage[n][M][H],
 *   f64 Z[n][cz], then per decomposition f64 U[n][n] and f64 lambda[n], f64 pheno[n][P], i64 column[T], i64 point[T].
 * Output: f64 lod[P][M], f64 peak_lod[P][n_chrom], i64 peak_index[P][n_chrom], f64 hsq[P][n_eig], i64 support_lo[P][n_chrom],
 *   i64 support_hi[P][n_chrom], then of the effects pass given those heritabilities f64 effect[T][H], f64 se[T][H],
 *   f64 lod[T], f64 sigma2[T], f64 hsq[T], i32 rank[T] (padded to 8 bytes), then f64 refused[T] of refused calls, which
 *   must have left the buffer as it was filled.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "gbrs_hip.h"

static void *xread(FILE *f, size_t n) {
    void *p = malloc(n ? n : 1);
    if (!p || fread(p, 1, n, f) != n) {
        fprintf(stderr, "scan_lmm_effects_client: short read\n");
        exit(2);
    }
    return p;
}

static void *xalloc(size_t n) {
    void *p = calloc(n ? n : 1, 1);
    if (!p) exit(2);
    return p;
}

#define CHECK(call)                                                              \
    do {                                                                         \
        const int st_ = (call);                                                  \
        if (st_ != GBRS_OK) {                                                    \
            fprintf(stderr, "scan_lmm_effects_client: %s -> %d: %s\n", #call, st_, gbrs_last_error()); \
            return 3;                                                            \
        }                                                                        \
    } while (0)

int main(int argc, char **argv) {
    if (argc != 3) return 1;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t head[6];
    int64_t P, T;
    double drop;
    if (fread(head, 4, 6, f) != 6 || fread(&P, 8, 1, f) != 1 || fread(&T, 8, 1, f) != 1 || fread(&drop, 8, 1, f) != 1) return 2;
    const int H = head[0], n_chrom = head[1], n = head[2], cz = head[3], n_eig = head[4];
    const int32_t *points = (const int32_t *)xread(f, ((size_t)n_chrom * 4 + 7) / 8 * 8);
    const int32_t *eig_of_chrom = (const int32_t *)xread(f, ((size_t)n_chrom * 4 + 7) / 8 * 8);
    int64_t M = 0, k;
    int c, e;
    for (c = 0; c < n_chrom; ++c) M += points[c];
    const double *dosage = (const double *)xread(f, (size_t)n * M * H * 8);
    const double *Z = (const double *)xread(f, (size_t)n * cz * 8);
    const double **U = (const double **)xalloc((size_t)n_eig * sizeof(double *));
    const double **lambda = (const double **)xalloc((size_t)n_eig * sizeof(double *));
    for (e = 0; e < n_eig; ++e) {
        U[e] = (const double *)xread(f, (size_t)n * n * 8);
        lambda[e] = (const double *)xread(f, (size_t)n * 8);
    }
    double *pheno = (double *)xread(f, (size_t)n * P * 8);
    int64_t *column = (int64_t *)xread(f, (size_t)T * 8), *point = (int64_t *)xread(f, (size_t)T * 8);
    fclose(f);

    const size_t PC = (size_t)(P * n_chrom), PE = (size_t)(P * n_eig), TH = (size_t)(T * H), rank_bytes = ((size_t)T * 4 + 7) / 8 * 8;
    gbrs_scan_t *scan = NULL;
    gbrs_scan_lmm_effects_info_t info;
    double *lod = (double *)xalloc((size_t)(P * M) * 8), *peak_lod = (double *)xalloc(PC * 8), *hsq = (double *)xalloc(PE * 8);
    int64_t *peak_index = (int64_t *)xalloc(PC * 8), *lo = (int64_t *)xalloc(PC * 8), *hi = (int64_t *)xalloc(PC * 8);
    double *effect = (double *)xalloc(TH * 8), *se = (double *)xalloc(TH * 8), *tlod = (double *)xalloc((size_t)T * 8);
    double *sigma2 = (double *)xalloc((size_t)T * 8), *thsq = (double *)xalloc((size_t)T * 8), *refused = (double *)xalloc((size_t)T * 8);
    int32_t *rank = (int32_t *)xalloc(rank_bytes);
    for (k = 0; k < T; ++k) refused[k] = -1.0;
    CHECK(gbrs_scan_create(0, n_chrom, points, H, &scan));
    CHECK(gbrs_scan_append(scan, n, dosage));
    /* not prepared */
    if (gbrs_scan_lmm_effects(scan, P, pheno, NULL, T, column, point, NULL, NULL, refused, NULL, NULL, NULL) != GBRS_ERR_INVALID) return 4;
    if (gbrs_scan_lmm_run_support(scan, P, pheno, NULL, drop, NULL, NULL, NULL, NULL, NULL, lo, hi) != GBRS_ERR_INVALID) return 4;
    CHECK(gbrs_scan_lmm_prepare(scan, cz, Z, n_eig, U, lambda, eig_of_chrom));
    if (gbrs_scan_lmm_run_support(scan, P, pheno, NULL, -1.0, NULL, NULL, NULL, NULL, NULL, lo, hi) != GBRS_ERR_INVALID) return 4;
    CHECK(gbrs_scan_lmm_run_support(scan, P, pheno, NULL, drop, lod, peak_lod, peak_index, hsq, NULL, lo, hi));
    column[0] += P;                                                               /* a column outside the table */
    if (gbrs_scan_lmm_effects(scan, P, pheno, hsq, T, column, point, NULL, NULL, refused, NULL, NULL, NULL) != GBRS_ERR_INVALID) return 4;
    column[0] -= P;
    point[T - 1] += M;                                                            /* a point outside the grid */
    if (gbrs_scan_lmm_effects(scan, P, pheno, hsq, T, column, point, NULL, NULL, refused, NULL, NULL, NULL) != GBRS_ERR_INVALID) return 4;
    point[T - 1] -= M;
    if (gbrs_scan_lmm_effects(scan, P, pheno, hsq, -1, column, point, NULL, NULL, refused, NULL, NULL, NULL) != GBRS_ERR_INVALID) return 4;
    CHECK(gbrs_scan_lmm_effects(scan, P, pheno, hsq, 0, NULL, NULL, NULL, NULL, refused, NULL, NULL, NULL));     /* T = 0: nothing */
    CHECK(gbrs_scan_lmm_effects(scan, P, pheno, hsq, T, column, point, effect, se, tlod, sigma2, rank, thsq));
    CHECK(gbrs_scan_lmm_effects_info(scan, &info));
    if (info.T != T || info.P != P || info.columns < 1 || info.columns > P || !(info.last_pass_ms > 0.0) || !(info.last_null_ms > 0.0) ||
        !(info.last_target_ms > 0.0) || info.peak_device_bytes == 0)
        return 5;
    printf("scan_lmm_effects_client: %lld targets of %lld columns, pass %.3f ms, null fits %.3f ms, targets %.3f ms\n", (long long)T,
           (long long)info.columns, info.last_pass_ms, info.last_null_ms, info.last_target_ms);
    f = fopen(argv[2], "wb");
    if (!f) return 2;
    fwrite(lod, 8, (size_t)(P * M), f);
    fwrite(peak_lod, 8, PC, f);
    fwrite(peak_index, 8, PC, f);
    fwrite(hsq, 8, PE, f);
    fwrite(lo, 8, PC, f);
    fwrite(hi, 8, PC, f);
    fwrite(effect, 8, TH, f);
    fwrite(se, 8, TH, f);
    fwrite(tlod, 8, (size_t)T, f);
    fwrite(sigma2, 8, (size_t)T, f);
    fwrite(thsq, 8, (size_t)T, f);
    fwrite(rank, 1, rank_bytes, f);
    fwrite(refused, 8, (size_t)T, f);
    fclose(f);
    CHECK(gbrs_scan_destroy(scan));
    return 0;
}
