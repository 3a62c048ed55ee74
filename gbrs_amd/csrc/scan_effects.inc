// Founder effects at QTL peaks and LOD support intervals on the scan handle (gbrs_scan_effects, gbrs_scan_run_support;
// DESIGN.md §31).  Included by scan.hip inside namespace gbrs, after scan_mediate.inc.  No fused multiply-add anywhere
// (-ffp-contract=off), no atomics, plain vector loads and stores.
//
// The rule of the effects, for target t with y = column[t] and m = point[t].  W_m = L^-1 X~' of gbrs_scan_prepare serves:
// no new factorisation of the design.
//   y~, rss0            by scan_pheno_kernel, as gbrs_scan_run forms them
//   S, r                the kept rows of W_m (a kept row has unit norm, a skipped one is zeros) and their number, rank[m]
//   a = W_S y~          r sums over the samples
//   X~_j, j < H - 1     founder j's dosage column at m with the covariates projected out: scan_prepare_kernel's steps 1-3
//   X~_{H-1}            by definition -sum_{j < H-1} X~_j: the sum constraint the scan assumes when it drops founder H - 1
//   R = W_S [X~_0 .. X~_{H-1}]   r x H; its last column is minus the sum of the others, j ascending
//   C = R R'            r x r, symmetric positive definite (R has full row rank): a plain Cholesky, no skip rule
//   effect = R' C^-1 a  the minimum-norm least-squares solution over all H founder columns
//   rss1 = max(rss0 - |a|^2, 0)      sigma2 = rss1 / (n - c - r)      se[h] = sqrt(sigma2) |C^-1 R[:, h]|
//   lod                 scan_lod(rss0, |a|^2, n / 2): gbrs_scan_run's formula and edge rules on this pass's sums
// With r = 0 every effect and se is 0.0.

constexpr int64_t SE_TCHUNK = 512;           // targets whose workspace rows are on the device at a time

// One workgroup per target of the chunk; its HP rows of x ([chunk][HP][n_ld]) are its workspace for X~'.  Every sum over
// the samples is one wavefront's in scan_prepare_kernel's order: lane l adds the samples l, l + 64, ... in order and the 64
// partial sums meet in wave_sum_all's butterfly, so the order depends on n alone.  The small dense part runs in LDS in a
// fixed order: thread 0 factors and solves for the effects, thread h < H solves for se[h].
//   1  x[j][s] = D[s][m][j] for the H - 1 kept founders           (scan_prepare_kernel's step 1)
//   2  qtx[k][j] = sum_s qz[s][k] x[j][s]                         (its step 2)
//   3  x[j][s] -= sum_k qz[s][k] qtx[k][j]                        (its step 3: X~, transposed)
//   4  per row i of W_m, one wavefront: R[i][j] = sum_s W_i[s] x[j][s] for every j, a[i] = sum_s W_i[s] y~[s], and
//      keep[i] = the row holds a value that is not zero
//   5  the dense part of the rule
template <int HP>
__global__ void __launch_bounds__(SC_THREADS)
scan_effects_kernel(int n, int64_t M, int H, int c, int64_t n_ld, double half_n, const double *__restrict__ D,
                    const double *__restrict__ qz, const double *__restrict__ W, const int32_t *__restrict__ rank,
                    const int64_t *__restrict__ column, const int64_t *__restrict__ point, const double *__restrict__ yt,
                    const double *__restrict__ rss0, double *__restrict__ x, double *__restrict__ effect,
                    double *__restrict__ se, double *__restrict__ lod, double *__restrict__ sigma2,
                    int32_t *__restrict__ rank_out) {
    constexpr int HF = HP + 1;                 // founders at most
    __shared__ double qtx[SC_MAX_C * HP];
    __shared__ double R[HP * HF], L[HP * HP], a[HP], z[HP], u[HF * HP], sd[1];
    __shared__ int keep[HP], rows[HP], kept[1];
    const int64_t t = blockIdx.x, m = point[t];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, Hx = H - 1;
    const double *w = W + m * HP * n_ld, *y = yt + column[t] * n_ld;
    double *xs = x + t * HP * n_ld;
    for (int idx = tid; idx < n * Hx; idx += SC_THREADS) {
        const int s = idx / Hx, j = idx % Hx;
        xs[j * n_ld + s] = D[((int64_t)s * M + m) * H + j];
    }
    __syncthreads();
    for (int q = wave; q < c * Hx; q += SC_THREADS / 64) {
        const int k = q / Hx, j = q % Hx;
        double acc = 0.0;
        for (int s = lane; s < n; s += 64) acc += qz[(int64_t)s * c + k] * xs[j * n_ld + s];
        acc = wave_sum_all(acc);
        if (lane == 0) qtx[k * HP + j] = acc;
    }
    __syncthreads();
    for (int idx = tid; idx < n * Hx; idx += SC_THREADS) {
        const int j = idx / n, s = idx % n;
        double p = 0.0;
        for (int k = 0; k < c; ++k) p += qz[(int64_t)s * c + k] * qtx[k * HP + j];
        xs[j * n_ld + s] -= p;
    }
    __syncthreads();
    for (int i = wave; i < Hx; i += SC_THREADS / 64) {
        double acc[HP], ay = 0.0;
#pragma unroll
        for (int j = 0; j < HP; ++j) acc[j] = 0.0;
        bool any = false;
        for (int s = lane; s < n; s += 64) {
            const double wv = w[i * n_ld + s];
            any |= wv != 0.0;
#pragma unroll
            for (int j = 0; j < HP; ++j)
                if (j < Hx) acc[j] += wv * xs[j * n_ld + s];
            ay += wv * y[s];
        }
#pragma unroll
        for (int j = 0; j < HP; ++j) {
            const double v = wave_sum_all(acc[j]);
            if (lane == 0 && j < Hx) R[i * HF + j] = v;
        }
        ay = wave_sum_all(ay);
        const bool row = __ballot(any) != 0;
        if (lane == 0) {
            a[i] = ay;
            keep[i] = row;
        }
    }
    __syncthreads();
    if (tid == 0) {
        int r = 0;
        for (int i = 0; i < Hx; ++i)
            if (keep[i]) rows[r++] = i;
        kept[0] = r;
        double ess = 0.0;
        for (int p = 0; p < r; ++p) {
            const int i = rows[p];
            double last = 0.0;
            for (int j = 0; j < Hx; ++j) last += R[i * HF + j];
            R[i * HF + Hx] = -last;
            ess += a[i] * a[i];
        }
        // C = R R' and its Cholesky factor, row by row
        for (int p = 0; p < r; ++p)
            for (int q = 0; q <= p; ++q) {
                double v = 0.0;
                for (int h = 0; h < H; ++h) v += R[rows[p] * HF + h] * R[rows[q] * HF + h];
                for (int k = 0; k < q; ++k) v -= L[p * HP + k] * L[q * HP + k];
                L[p * HP + q] = p == q ? sqrt(v) : v / L[q * HP + q];
            }
        // z = C^-1 a: forward, then backward
        for (int p = 0; p < r; ++p) {
            double v = a[rows[p]];
            for (int k = 0; k < p; ++k) v -= L[p * HP + k] * z[k];
            z[p] = v / L[p * HP + p];
        }
        for (int p = r - 1; p >= 0; --p) {
            double v = z[p];
            for (int k = p + 1; k < r; ++k) v -= L[k * HP + p] * z[k];
            z[p] = v / L[p * HP + p];
        }
        const double rss = rss0[column[t]];
        const double rss1 = rss - ess > 0.0 ? rss - ess : 0.0;
        const double s2 = rss1 / (double)(n - c - rank[m]);
        sd[0] = sqrt(s2);
        lod[t] = scan_lod(rss, ess, half_n);
        sigma2[t] = s2;
        rank_out[t] = rank[m];
    }
    __syncthreads();
    if (tid < H) {
        const int h = tid, r = kept[0];
        double *v = u + h * HP, e = 0.0, norm = 0.0;
        for (int p = 0; p < r; ++p) {
            double b = R[rows[p] * HF + h];
            for (int k = 0; k < p; ++k) b -= L[p * HP + k] * v[k];
            v[p] = b / L[p * HP + p];
        }
        for (int p = r - 1; p >= 0; --p) {
            double b = v[p];
            for (int k = p + 1; k < r; ++k) b -= L[k * HP + p] * v[k];
            v[p] = b / L[p * HP + p];
        }
        for (int p = 0; p < r; ++p) {
            e += R[rows[p] * HF + h] * z[p];
            norm += v[p] * v[p];
        }
        effect[t * H + h] = e;
        se[t * H + h] = sd[0] * sqrt(norm);
    }
}

// ---- LOD support intervals -----------------------------------------------------------------------------------------------------

// One wavefront per (chromosome, phenotype of the chunk), after scan_peak_kernel on the chunk's LOD rows.  With the peak
// index k, its value v and the bound v - drop (the one subtraction): support_lo is the largest index i < k of the
// chromosome with lod[i] <= v - drop, the chromosome's first point without one; support_hi the smallest i > k, the last
// point without one; -1 both for a chromosome without points.  The wavefront walks outward from k 64 points at a time -
// lane l looks at k - base - l (k + base + l), so lane 0 of the first step stands on k itself and is not counted - and a
// ballot finds the nearest lane that has fallen.
__global__ void __launch_bounds__(64)
scan_support_kernel(int64_t M, int n_chrom, double drop, const int64_t *__restrict__ point_off, const double *__restrict__ lod,
                    const double *__restrict__ peak_lod, const int64_t *__restrict__ peak_index,
                    int64_t *__restrict__ support_lo, int64_t *__restrict__ support_hi) {
    const int c = blockIdx.x, lane = threadIdx.x;
    const int64_t p = blockIdx.y, first = point_off[c], last = point_off[c + 1] - 1, k = peak_index[p * n_chrom + c];
    if (k < 0) {
        if (lane == 0) support_lo[p * n_chrom + c] = support_hi[p * n_chrom + c] = -1;
        return;
    }
    const double bound = peak_lod[p * n_chrom + c] - drop;
    const double *row = lod + p * M;
    int64_t lo = first, hi = last;
    for (int64_t base = 0; k - base >= first; base += 64) {
        const int64_t i = k - base - lane;
        const unsigned long long fallen = __ballot(i < k && i >= first && row[i] <= bound);
        if (fallen) {
            lo = k - base - (__ffsll(fallen) - 1);
            break;
        }
    }
    for (int64_t base = 0; k + base <= last; base += 64) {
        const int64_t i = k + base + lane;
        const unsigned long long fallen = __ballot(i > k && i <= last && row[i] <= bound);
        if (fallen) {
            hi = k + base + (__ffsll(fallen) - 1);
            break;
        }
    }
    if (lane == 0) {
        support_lo[p * n_chrom + c] = lo;
        support_hi[p * n_chrom + c] = hi;
    }
}
