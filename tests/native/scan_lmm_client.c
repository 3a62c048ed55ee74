/* A plain C99 client of the mixed-model genome scan (include/gbrs_hip.h: gbrs_scan_create, _append, _kinship,
 * _lmm_prepare, _lmm_run, _lmm_ranks, _lmm_info).  tests/test_scan_lmm_client.py compiles it with gcc -std=c99 -pedantic
 * -Werror, links it against gbrs_amd/libgbrs_hip.so and compares its output with the numpy restatements.  The client
 * brings its own decompositions: it reads them from the fixture the test writes.
 *
 * Input (little endian): i32 H, i32 n_chrom, i32 n, i32 cz, i32 n_eig, i32 leave_out, i64 P, f64 scale,
 *   i32 points[n_chrom] (padded to 8 bytes), i32 eig_of_chrom[n_chrom] (padded to 8 bytes), f64 dosage[n][M][H],
 *   f64 Z[n][cz], then per decomposition f64 U[n][n] and f64 lambda[n], f64 pheno[n][P].
 * Output: f64 K[n][n], f64 lod[P][M], f64 peak_lod[P][n_chrom], i64 peak_index[P][n_chrom], f64 hsq[P][n_eig],
 *   f64 sigma2[P][n_eig], i32 rank_min[P], i32 rank_max[P] (together padded to 8 bytes), then a second hsq[P][n_eig] of
 *   refused calls, which must have left the buffer as it was filled.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "gbrs_hip.h"

static void *xread(FILE *f, size_t n) {
    void *p = malloc(n ? n : 1);
    if (!p || fread(p, 1, n, f) != n) {
        fprintf(stderr, "scan_lmm_client: short read\n");
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
            fprintf(stderr, "scan_lmm_client: %s -> %d: %s\n", #call, st_, gbrs_last_error()); \
            return 3;                                                            \
        }                                                                        \
    } while (0)

int main(int argc, char **argv) {
    if (argc != 3) return 1;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t head[6];
    int64_t P;
    double scale;
    if (fread(head, 4, 6, f) != 6 || fread(&P, 8, 1, f) != 1 || fread(&scale, 8, 1, f) != 1) return 2;
    const int H = head[0], n_chrom = head[1], n = head[2], cz = head[3], n_eig = head[4], leave_out = head[5];
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
    fclose(f);

    const size_t PC = (size_t)(P * n_chrom), PE = (size_t)(P * n_eig), rank_bytes = ((size_t)P * 8 + 7) / 8 * 8;
    gbrs_scan_t *scan = NULL;
    gbrs_scan_lmm_info_t info;
    double *K = (double *)xalloc((size_t)n * n * 8), *lod = (double *)xalloc((size_t)(P * M) * 8);
    double *peak_lod = (double *)xalloc(PC * 8), *hsq = (double *)xalloc(PE * 8), *sigma2 = (double *)xalloc(PE * 8);
    double *refused = (double *)xalloc(PE * 8), *bad = (double *)xalloc(PE * 8);
    int64_t *peak_index = (int64_t *)xalloc(PC * 8);
    int32_t *rank = (int32_t *)xalloc(rank_bytes);
    for (k = 0; k < (int64_t)PE; ++k) {
        refused[k] = -1.0;
        bad[k] = 0.5;
    }
    bad[PE - 1] = 1.25;                                                           /* a heritability outside [0, 1] */
    CHECK(gbrs_scan_create(0, n_chrom, points, H, &scan));
    CHECK(gbrs_scan_append(scan, n, dosage));
    if (gbrs_scan_lmm_run(scan, P, pheno, NULL, NULL, NULL, NULL, refused, NULL) != GBRS_ERR_INVALID) return 4;   /* not prepared */
    if (gbrs_scan_kinship(scan, n_chrom, scale, K) != GBRS_ERR_INVALID) return 4;  /* no such chromosome */
    CHECK(gbrs_scan_kinship(scan, leave_out, scale, K));
    if (gbrs_scan_lmm_prepare(scan, 17, Z, n_eig, U, lambda, eig_of_chrom) != GBRS_ERR_INVALID) return 4;
    CHECK(gbrs_scan_lmm_prepare(scan, cz, Z, n_eig, U, lambda, eig_of_chrom));
    if (gbrs_scan_lmm_run(scan, P, pheno, bad, NULL, NULL, NULL, refused, NULL) != GBRS_ERR_INVALID) return 4;
    CHECK(gbrs_scan_lmm_run(scan, P, pheno, NULL, lod, peak_lod, peak_index, hsq, sigma2));
    CHECK(gbrs_scan_lmm_ranks(scan, rank, rank + P));
    CHECK(gbrs_scan_lmm_info(scan, &info));
    if (info.cz != cz || info.n_eig != n_eig || info.P != P || !(info.last_kinship_ms > 0.0) || !(info.last_rotate_ms > 0.0) ||
        !(info.last_null_ms > 0.0) || !(info.last_point_ms > 0.0) || info.device_bytes == 0 ||
        info.peak_device_bytes <= info.device_bytes)
        return 5;
    printf("scan_lmm_client: %lld phenotypes, kinship %.3f ms, rotation %.3f ms, null fits %.3f ms, weighted scan %.3f ms\n",
           (long long)P, info.last_kinship_ms, info.last_rotate_ms, info.last_null_ms, info.last_point_ms);
    f = fopen(argv[2], "wb");
    if (!f) return 2;
    fwrite(K, 8, (size_t)n * n, f);
    fwrite(lod, 8, (size_t)(P * M), f);
    fwrite(peak_lod, 8, PC, f);
    fwrite(peak_index, 8, PC, f);
    fwrite(hsq, 8, PE, f);
    fwrite(sigma2, 8, PE, f);
    fwrite(rank, 1, rank_bytes, f);
    fwrite(refused, 8, PE, f);
    fclose(f);
    CHECK(gbrs_scan_destroy(scan));
    return 0;
}
