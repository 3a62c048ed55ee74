/* A plain C99 client of the genome scan with interactive covariates (include/gbrs_hip.h: gbrs_scan_create, _append,
 * _int_prepare, _int_run, _int_info).  tests/test_scan_int_client.py compiles it with gcc -std=c99 -pedantic -Werror, links
 * it against gbrs_amd/libgbrs_hip.so and compares its output with the numpy restatements.  The client brings its own
 * covariate basis: it reads it from the fixture the test writes.
 *
 * Input (little endian): i32 H, i32 n_chrom, i32 n, i32 c, i32 k, i32 0, i64 P, i32 points[n_chrom] (padded to 8 bytes),
 *   f64 dosage[n][M][H], f64 qz[n][c], f64 zint[n][k], f64 pheno[n][P].
 * Output: f64 lod_full[P][M], f64 lod_add[P][M], f64 lod_int[P][M], f64 peak_full[P][n_chrom], i64 peak_full_index[P][n_chrom],
 *   f64 peak_full_add[P][n_chrom], f64 peak_int[P][n_chrom], i64 peak_int_index[P][n_chrom], i32 rank_full[M], i32 rank_add[M]
 *   (together padded to 8 bytes), then a second peak_int[P][n_chrom] of refused calls, which must have left the buffer as
 *   it was filled.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "gbrs_hip.h"

static void *xread(FILE *f, size_t n) {
    void *p = malloc(n ? n : 1);
    if (!p || fread(p, 1, n, f) != n) {
        fprintf(stderr, "scan_int_client: short read\n");
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
            fprintf(stderr, "scan_int_client: %s -> %d: %s\n", #call, st_, gbrs_last_error()); \
            return 3;                                                            \
        }                                                                        \
    } while (0)

int main(int argc, char **argv) {
    if (argc != 3) return 1;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t head[6];
    int64_t P;
    if (fread(head, 4, 6, f) != 6 || fread(&P, 8, 1, f) != 1) return 2;
    const int H = head[0], n_chrom = head[1], n = head[2], c = head[3], k = head[4];
    const int32_t *points = (const int32_t *)xread(f, ((size_t)n_chrom * 4 + 7) / 8 * 8);
    int64_t M = 0, q;
    int ch;
    for (ch = 0; ch < n_chrom; ++ch) M += points[ch];
    const double *dosage = (const double *)xread(f, (size_t)n * M * H * 8);
    const double *qz = (const double *)xread(f, (size_t)n * c * 8);
    const double *zint = (const double *)xread(f, (size_t)n * k * 8);
    const double *pheno = (const double *)xread(f, (size_t)n * P * 8);
    fclose(f);

    const size_t PM = (size_t)(P * M), PC = (size_t)(P * n_chrom), rank_bytes = ((size_t)M * 8 + 7) / 8 * 8;
    gbrs_scan_t *scan = NULL;
    gbrs_scan_int_info_t info;
    double *lod_full = (double *)xalloc(PM * 8), *lod_add = (double *)xalloc(PM * 8), *lod_int = (double *)xalloc(PM * 8);
    double *peak_full = (double *)xalloc(PC * 8), *peak_full_add = (double *)xalloc(PC * 8), *peak_int = (double *)xalloc(PC * 8);
    double *refused = (double *)xalloc(PC * 8);
    int64_t *peak_full_index = (int64_t *)xalloc(PC * 8), *peak_int_index = (int64_t *)xalloc(PC * 8);
    int32_t *rank = (int32_t *)xalloc(rank_bytes);
    for (q = 0; q < (int64_t)PC; ++q) refused[q] = -1.0;
    CHECK(gbrs_scan_create(0, n_chrom, points, H, &scan));
    CHECK(gbrs_scan_append(scan, n, dosage));
    if (gbrs_scan_int_run(scan, P, pheno, NULL, NULL, NULL, NULL, NULL, NULL, refused, NULL) != GBRS_ERR_INVALID) return 4; /* not prepared */
    if (gbrs_scan_int_prepare(scan, c, qz, 0, zint) != GBRS_ERR_INVALID) return 4;                     /* no interactive covariate */
    if (gbrs_scan_int_prepare(scan, 65, qz, k, zint) != GBRS_ERR_INVALID) return 4;
    if (gbrs_scan_int_prepare(scan, c, qz, 64, zint) != GBRS_ERR_UNSUPPORTED) return 4;                /* more than 64 rows */
    CHECK(gbrs_scan_int_prepare(scan, c, qz, k, zint));
    if (gbrs_scan_int_run(scan, 0, pheno, NULL, NULL, NULL, NULL, NULL, NULL, refused, NULL) != GBRS_ERR_INVALID) return 4;
    CHECK(gbrs_scan_int_run(scan, P, pheno, lod_full, lod_add, lod_int, peak_full, peak_full_index, peak_full_add, peak_int,
                            peak_int_index));
    CHECK(gbrs_scan_int_info(scan, &info, rank, rank + M));
    if (info.n != n || info.M != M || info.H != H || info.c != c || info.k != k || (info.HPI != 16 && info.HPI != 32 && info.HPI != 64) ||
        !(info.last_prepare_ms > 0.0) || !(info.last_run_ms >= info.last_product_ms) || !(info.last_product_ms > 0.0) ||
        info.device_bytes == 0)
        return 5;
    printf("scan_int_client: %lld phenotypes, %d rows per grid point, prepare %.3f ms, run %.3f ms, product %.3f ms\n", (long long)P,
           (int)info.HPI, info.last_prepare_ms, info.last_run_ms, info.last_product_ms);
    f = fopen(argv[2], "wb");
    if (!f) return 2;
    fwrite(lod_full, 8, PM, f);
    fwrite(lod_add, 8, PM, f);
    fwrite(lod_int, 8, PM, f);
    fwrite(peak_full, 8, PC, f);
    fwrite(peak_full_index, 8, PC, f);
    fwrite(peak_full_add, 8, PC, f);
    fwrite(peak_int, 8, PC, f);
    fwrite(peak_int_index, 8, PC, f);
    fwrite(rank, 1, rank_bytes, f);
    fwrite(refused, 8, PC, f);
    fclose(f);
    CHECK(gbrs_scan_destroy(scan));
    return 0;
}
