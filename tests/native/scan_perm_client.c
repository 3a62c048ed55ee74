/* A plain C99 client of the genome scan's permutation pass (include/gbrs_hip.h: gbrs_scan_create, _append, _prepare,
 * _permute, _perm_info).  tests/test_scan_perm_client.py compiles it with gcc -std=c99 -pedantic -Werror, links it
 * against gbrs_amd/libgbrs_hip.so and compares its output with the numpy restatement of the rule.
 *
 * Input (little endian): i32 H, i32 n_chrom, i32 n, i32 c, i64 P, i64 B, u64 seed, i32 points[n_chrom] (padded to 8
 *   bytes), u8 mask[n_chrom] (padded to 8 bytes), f64 dosage[n][M][H], f64 qz[n][c], f64 pheno[n][P].
 * Output: f64 perm_max[P][B], i32 perm_index[B][n], then a second perm_max[P][B] of a refused call (B = 0), which must
 *   have left the buffer as it was filled.
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "gbrs_hip.h"

static void *xread(FILE *f, size_t n) {
    void *p = malloc(n ? n : 1);
    if (!p || fread(p, 1, n, f) != n) {
        fprintf(stderr, "scan_perm_client: short read\n");
        exit(2);
    }
    return p;
}

#define CHECK(call)                                                              \
    do {                                                                         \
        const int st_ = (call);                                                  \
        if (st_ != GBRS_OK) {                                                    \
            fprintf(stderr, "scan_perm_client: %s -> %d: %s\n", #call, st_, gbrs_last_error()); \
            return 3;                                                            \
        }                                                                        \
    } while (0)

int main(int argc, char **argv) {
    if (argc != 3) return 1;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    int32_t head[4];
    int64_t size[2];
    uint64_t seed;
    if (fread(head, 4, 4, f) != 4 || fread(size, 8, 2, f) != 2 || fread(&seed, 8, 1, f) != 1) return 2;
    const int H = head[0], n_chrom = head[1], n = head[2], c = head[3];
    const int64_t P = size[0], B = size[1];
    const int32_t *points = (const int32_t *)xread(f, ((size_t)n_chrom * 4 + 7) / 8 * 8);
    const uint8_t *mask = (const uint8_t *)xread(f, ((size_t)n_chrom + 7) / 8 * 8);
    int64_t M = 0, k;
    int ch;
    for (ch = 0; ch < n_chrom; ++ch) M += points[ch];
    const double *dosage = (const double *)xread(f, (size_t)n * M * H * 8);
    const double *qz = (const double *)xread(f, (size_t)n * c * 8);
    const double *pheno = (const double *)xread(f, (size_t)n * P * 8);
    fclose(f);

    gbrs_scan_t *scan = NULL;
    gbrs_scan_perm_info_t info;
    double *perm_max = (double *)malloc((size_t)(P * B) * 8), *refused = (double *)malloc((size_t)(P * B) * 8);
    int32_t *perm_index = (int32_t *)malloc((size_t)(B * n) * 4);
    if (!perm_max || !refused || !perm_index) return 2;
    for (k = 0; k < P * B; ++k) refused[k] = -1.0;
    CHECK(gbrs_scan_create(0, n_chrom, points, H, &scan));
    CHECK(gbrs_scan_append(scan, n, dosage));
    if (gbrs_scan_permute(scan, P, pheno, B, seed, mask, refused, NULL) != GBRS_ERR_INVALID) return 4;   /* not prepared */
    CHECK(gbrs_scan_prepare(scan, c, qz));
    if (gbrs_scan_permute(scan, P, pheno, 0, seed, mask, refused, NULL) != GBRS_ERR_INVALID) return 4;
    CHECK(gbrs_scan_permute(scan, P, pheno, B, seed, mask, perm_max, perm_index));
    CHECK(gbrs_scan_perm_info(scan, &info));
    if (info.P != P || info.B != B || !(info.last_permute_ms >= info.last_product_ms) || !(info.last_product_ms > 0.0)) return 5;
    printf("scan_perm_client: %lld x %lld columns, pass %.3f ms, product %.3f ms, %llu bytes at the peak\n", (long long)P,
           (long long)B, info.last_permute_ms, info.last_product_ms, (unsigned long long)info.peak_device_bytes);
    f = fopen(argv[2], "wb");
    if (!f) return 2;
    fwrite(perm_max, 8, (size_t)(P * B), f);
    fwrite(perm_index, 4, (size_t)(B * n), f);
    fwrite(refused, 8, (size_t)(P * B), f);
    fclose(f);
    CHECK(gbrs_scan_destroy(scan));
    return 0;
}
