// Interactive covariates of the genome scan (gbrs_scan_int_*; DESIGN.md §35), included by scan.hip inside namespace gbrs.
//
// k interactive covariates zint [n][k] add k (H - 1) columns to a grid point's design, after the additive ones:
//   column col < Hx:               x[s] = D[s][m][col]
//   column Hx + q Hx + j:          x[s] = D[s][m][j] zint[s][q]
// and §27's factorisation - raw, projection on qz, Gram matrix, Cholesky with the skip rule - runs over all of them in that
// order.  The leading rows of the new W are therefore the plain scan's W, bit for bit, and one product gives the explained
// sums of squares of the additive model (the first Hp rows) and of the full model (all rows).
//
// Storage: W is [M * HPI][n_ld].  A point's first Hp rows are plain W's (Hx additive rows, then zeros), the k Hx interaction
// rows follow from row Hp, zeros up to HPI = 16, 32 or 64.  No 48-row variant: a 64-row tile would hold one point and a
// third, so a point's wavefronts would no longer lie in one workgroup; it would serve Hp + k Hx in 33 .. 48 only (H = 8, 9
// with k = 4, 5 and H >= 10 with k = 2), and there the product is not the larger part of a run.

// The row of W a design column lives in.
__device__ __forceinline__ int scan_int_row(int col, int Hx, int Hp) { return col < Hx ? col : col + (Hp - Hx); }

// One workgroup per grid point m, as scan_prepare_kernel, over NC = Hx (1 + k) <= HPI columns; every sum over the samples
// is formed in its order (one wavefront, lane l adds the samples l, l + 64, ..., then the butterfly), so the additive
// columns go through the same operations on the same numbers.
//   1  the columns as built, zeros elsewhere
//   2  qtx[c'][col] = sum_s qz[s][c'] x_col[s], raw[col] = sum_s x_col[s]^2
//   3  x_col[s] -= sum_c' qz[s][c'] qtx[c'][col]
//   4  G[col][i] = sum_s x_col[s] x_i[s], i <= col: the packed lower triangle T
//   5  Cholesky with the skip rule, in place: L over G's triangle.  Column after column; within a column the rows below the
//      diagonal are one thread each.  Row j's entry of column i is (G_ji - sum over the kept t < i of L_jt L_it) / L_ii with
//      t ascending, and d_j = G_jj - sum over the kept i < j of L_ji^2 with i ascending: the one-thread factorisation's
//      operations in its order, whoever performs them
//   6  per sample, forward substitution down the kept columns; a thread reads back only what it wrote itself
// LDS per workgroup, c up to 64 covariates: qtx 64 HPI doubles, T HPI (HPI + 1) / 2 doubles, raw HPI doubles, keep HPI
// ints: 9.4 KB at HPI = 16, 20.6 KB at 32, 49.0 KB at 64.
template <int HPI>
__global__ void __launch_bounds__(SC_THREADS)
scan_int_prepare_kernel(int n, int64_t M, int H, int Hp, int c, int k, int64_t n_ld, const double *__restrict__ D,
                        const double *__restrict__ qz, const double *__restrict__ zint, double *__restrict__ W,
                        int32_t *__restrict__ rank_full, int32_t *__restrict__ rank_add) {
    __shared__ double qtx[SC_MAX_C * HPI];
    __shared__ double T[HPI * (HPI + 1) / 2], raw[HPI];
    __shared__ int keep[HPI];
    const int64_t m = blockIdx.x;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, Hx = H - 1, NC = Hx * (1 + k);
    double *w = W + m * HPI * n_ld;
    for (int64_t idx = tid; idx < HPI * n_ld; idx += SC_THREADS) {
        const int row = (int)(idx / n_ld), s = (int)(idx % n_ld);
        double v = 0.0;
        if (s < n) {
            if (row < Hx) v = D[((int64_t)s * M + m) * H + row];
            else if (row >= Hp && row < Hp + k * Hx) {
                const int q = (row - Hp) / Hx, j = (row - Hp) % Hx;
                v = D[((int64_t)s * M + m) * H + j] * zint[(int64_t)s * k + q];
            }
        }
        w[idx] = v;
    }
    __syncthreads();
    for (int q = wave; q < (c + 1) * NC; q += SC_THREADS / 64) {
        const int kc = q / NC, col = q % NC;
        const double *x = w + scan_int_row(col, Hx, Hp) * n_ld;
        double acc = 0.0;
        if (kc < c)
            for (int s = lane; s < n; s += 64) acc += qz[(int64_t)s * c + kc] * x[s];
        else
            for (int s = lane; s < n; s += 64) acc += x[s] * x[s];
        acc = wave_sum_all(acc);
        if (lane == 0) (kc < c ? qtx[kc * HPI + col] : raw[col]) = acc;
    }
    __syncthreads();
    for (int idx = tid; idx < n * NC; idx += SC_THREADS) {
        const int col = idx / n, s = idx % n;
        double p = 0.0;
        for (int kc = 0; kc < c; ++kc) p += qz[(int64_t)s * c + kc] * qtx[kc * HPI + col];
        w[scan_int_row(col, Hx, Hp) * n_ld + s] -= p;
    }
    __syncthreads();
    for (int q = wave; q < NC * (NC + 1) / 2; q += SC_THREADS / 64) {
        int j = 0;
        while ((j + 1) * (j + 2) / 2 <= q) ++j;
        const int i = q - j * (j + 1) / 2;
        const double *xj = w + scan_int_row(j, Hx, Hp) * n_ld, *xi = w + scan_int_row(i, Hx, Hp) * n_ld;
        double acc = 0.0;
        for (int s = lane; s < n; s += 64) acc += xj[s] * xi[s];
        acc = wave_sum_all(acc);
        if (lane == 0) T[j * (j + 1) / 2 + i] = acc;
    }
    __syncthreads();
    for (int i = 0; i < NC; ++i) {
        if (tid == 0) {
            const double gii = T[i * (i + 1) / 2 + i];
            double d = gii;
            for (int t = 0; t < i; ++t)
                if (keep[t]) {
                    const double v = T[i * (i + 1) / 2 + t];
                    d -= v * v;
                }
            const int ok = gii > SC_PIVOT * raw[i] && d > SC_PIVOT * gii;
            keep[i] = ok;
            if (ok) T[i * (i + 1) / 2 + i] = sqrt(d);
            else
                for (int t = 0; t <= i; ++t) T[i * (i + 1) / 2 + t] = 0.0;
        }
        __syncthreads();
        const int j = i + 1 + tid;
        if (j < NC) {
            double v = 0.0;
            if (keep[i]) {
                v = T[j * (j + 1) / 2 + i];
                for (int t = 0; t < i; ++t)
                    if (keep[t]) v -= T[j * (j + 1) / 2 + t] * T[i * (i + 1) / 2 + t];
                v /= T[i * (i + 1) / 2 + i];
            }
            T[j * (j + 1) / 2 + i] = v;
        }
        __syncthreads();
    }
    if (tid == 0) {
        int kept_add = 0, kept = 0;
        for (int j = 0; j < NC; ++j) {
            kept += keep[j];
            if (j < Hx) kept_add += keep[j];
        }
        rank_full[m] = kept;
        rank_add[m] = kept_add;
    }
    for (int s = tid; s < n; s += SC_THREADS)
        for (int j = 0; j < NC; ++j) {
            double *xj = w + scan_int_row(j, Hx, Hp) * n_ld;
            double v = 0.0;
            if (keep[j]) {
                v = xj[s];
                for (int i = 0; i < j; ++i)
                    if (keep[i]) v -= T[j * (j + 1) / 2 + i] * w[scan_int_row(i, Hx, Hp) * n_ld + s];
                v /= T[j * (j + 1) / 2 + j];
            }
            xj[s] = v;
        }
}

// lod_int of DESIGN.md §35 from the two explained sums of squares, ess_full >= ess_add: never negative, never NaN.
__device__ __forceinline__ double scan_int_lod(double rss0, double ess_add, double ess_full, double half_n) {
    const double rss_add = rss0 - ess_add, rss_full = rss0 - ess_full;
    if (rss0 == 0.0 || rss_add <= 0.0) return 0.0;
    if (rss_full <= 0.0) return __builtin_huge_val();
    return half_n * log10(rss_add / rss_full);
}

// scan_lod_kernel's sibling over the rows of the new W: the same 64 x 64 x 32 tile, operand maps, LDS stride, prefetch and
// K chain, so a row's dot product with a column has the plain kernel's bits.  A grid point's HPI rows are those of WPP = HPI
// / 16 wavefronts of one workgroup, which holds 64 / HPI points.
// Epilogue: every wavefront squares and adds its 16 rows in the plain kernel's order - register order in the lane, then
// xor 16, then xor 32.  The first wavefront of a point holds the additive Hp rows: at Hp = 8 they are registers 0, 1 and the
// interaction rows that share its 16 are registers 2, 3, two sums; at Hp = 16 all four registers are additive.  The sums
// go to LDS as [column][wavefront] (additive) and [column][wavefront] (interaction), and one thread per (column, point)
// adds the interaction sums in wavefront order: ess_add is the plain kernel's ess, ess_full = ess_add + ess_x.  No atomics.
// Up to three LOD rows are stored per (phenotype, point), each where its pointer is not NULL.
template <int HPI>
__global__ void __launch_bounds__(SC_THREADS)
scan_int_lod_kernel(int64_t M, int64_t P, int64_t n_ld, int Hp, double half_n, const double *__restrict__ W,
                    const double *__restrict__ yt, const double *__restrict__ rss0, double *__restrict__ lod_full,
                    double *__restrict__ lod_add, double *__restrict__ lod_int) {
    constexpr int PTS = SC_ROWS / HPI, WPP = HPI / 16;     // grid points per workgroup, wavefronts per point
    __shared__ __attribute__((aligned(16))) double lds_a[SC_ROWS * SC_LD];
    __shared__ __attribute__((aligned(16))) double lds_b[SC_COLS * SC_LD];
    const int64_t row0 = (int64_t)blockIdx.x * SC_ROWS, col0 = (int64_t)blockIdx.y * SC_COLS, rows = M * HPI;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, i = lane & 15, g = lane >> 4;
    scan_d4 acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = scan_d4{0.0, 0.0, 0.0, 0.0};
    const double *ra = lds_a + (wave * 16 + i) * SC_LD + g, *rb = lds_b + i * SC_LD + g;
    auto multiply = [&]() {
#pragma unroll
        for (int kk = 0; kk < SC_KC; kk += 4) {
            const double av = ra[kk];
#pragma unroll
            for (int t = 0; t < 4; ++t) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, rb[t * 16 * SC_LD + kk], acc[t], 0, 0, 0);
        }
    };
    const int64_t chunks = n_ld / SC_KC;       // >= 1
    double va[SC_PER], vb[SC_PER];
    scan_fetch(va, W, n_ld, row0, rows);
    scan_fetch(vb, yt, n_ld, col0, P);
    for (int64_t kc = 1; kc < chunks; ++kc) {
        scan_put(lds_a, va);
        scan_put(lds_b, vb);
        __syncthreads();
        scan_fetch(va, W + kc * SC_KC, n_ld, row0, rows);
        scan_fetch(vb, yt + kc * SC_KC, n_ld, col0, P);
        multiply();
        __syncthreads();
    }
    scan_put(lds_a, va);
    scan_put(lds_b, vb);
    __syncthreads();
    multiply();
    __syncthreads();
    double *ess_a = lds_a, *ess_x = lds_a + SC_COLS * 4;       // [64 columns][4 wavefronts] each
    const bool first = wave % WPP == 0;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const double lo = acc[t][0] * acc[t][0] + acc[t][1] * acc[t][1];
        double ea, ex;
        if (first && Hp == 8) {
            ea = lo;
            ex = acc[t][2] * acc[t][2] + acc[t][3] * acc[t][3];
        } else {
            const double all = (lo + acc[t][2] * acc[t][2]) + acc[t][3] * acc[t][3];
            ea = first ? all : 0.0;
            ex = first ? 0.0 : all;
        }
        ea += __shfl_xor(ea, 16, WAVE);
        ea += __shfl_xor(ea, 32, WAVE);
        ex += __shfl_xor(ex, 16, WAVE);
        ex += __shfl_xor(ex, 32, WAVE);
        if (g == 0) {
            ess_a[(t * 16 + i) * 4 + wave] = ea;
            ess_x[(t * 16 + i) * 4 + wave] = ex;
        }
    }
    __syncthreads();
    if (threadIdx.x < SC_COLS * PTS) {
        const int col = threadIdx.x / PTS, pt = threadIdx.x % PTS;
        const int64_t m = (int64_t)blockIdx.x * PTS + pt, p = col0 + col;
        if (m < M && p < P) {
            const double add = ess_a[col * 4 + pt * WPP];
            double x = ess_x[col * 4 + pt * WPP];
#pragma unroll
            for (int v = 1; v < WPP; ++v) x += ess_x[col * 4 + pt * WPP + v];
            const double full = add + x, r0 = rss0[p];
            if (lod_full) lod_full[p * M + m] = scan_lod(r0, full, half_n);
            if (lod_add) lod_add[p * M + m] = scan_lod(r0, add, half_n);
            if (lod_int) lod_int[p * M + m] = scan_int_lod(r0, add, full, half_n);
        }
    }
}

// lod_add at the full model's peaks: one thread per (phenotype of the chunk, chromosome); NaN for a chromosome without points.
__global__ void __launch_bounds__(64)
scan_int_peak_add_kernel(int64_t M, int64_t count, int n_chrom, const int64_t *__restrict__ peak_index,
                         const double *__restrict__ lod_add, double *__restrict__ peak_add) {
    const int64_t q = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (q >= count) return;
    const int64_t at = peak_index[q];
    peak_add[q] = at < 0 ? __builtin_nan("") : lod_add[q / n_chrom * M + at];
}
