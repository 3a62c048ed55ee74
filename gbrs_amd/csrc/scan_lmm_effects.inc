// Founder effects at QTL peaks under the mixed model on the scan handle (gbrs_scan_lmm_effects; DESIGN.md §34).  Included by
// scan.hip inside namespace gbrs, after scan_lmm_snp.inc.  No fused multiply-add anywhere (-ffp-contract=off), no atomics,
// plain vector loads and stores.
//
// The rule of the effects, for target t with y = column[t] and m = point[t]; e is the decomposition of m's chromosome and h
// the heritability of (y, e), fitted by §32's search or given:
//   sw, Qz, y~, rss0     what lmm_null_kernel leaves for (y, e): w = v^-1/2, Z^ after Gram-Schmidt, the projected y^
//   X^_j = sw . R_m[j],  j < H-1;   raw_j = |X^_j|^2;   X~_j = X^_j - Qz Qz' X^_j      (lmm_point_kernel's steps 1-3)
//   G = X~' X~,  b = X~' y~                                                             (its step 4)
//   L, S, r              Cholesky of G with §27's skip rule, both lines of it; S the kept columns, r their number (step 5)
//   a = L_S^-1 b_S,      ess = |a|^2
//   R = L_S^-1 G[S, 0:H-1]   (r x (H-1));   R[:, H-1] = -sum_{j<H-1} R[:, j], j ascending        -> r x H
//   C = R R'             r x r, symmetric positive definite: a plain Cholesky, no skip rule
//   effect = R' C^-1 a   the minimum-norm generalised-least-squares solution over all H founder columns
//   rss1 = max(rss0 - ess, 0)     sigma2 = rss1 / (n - cz - r)     se[h] = sqrt(sigma2) |C^-1 R[:, h]|
//   lod = scan_lod(rss0, ess, n / 2)
// The last column is §31's definition carried over: the projected weighted column of founder H-1 is minus the sum of the
// others.  The rotated, weighted constant lies in the span of Qz, so this is what the sum constraint of the dosages implies,
// and it keeps the rule defined where a row does not add up.  R's first H-1 columns come from the Gram matrix: no sum over
// the samples beyond those of steps 2 and 4.  With r = 0 every effect and se is 0.0 and so is the LOD, while sigma2 stays
// the null model's, rss0 / (n - cz), as the formula gives it; a column of zeros gives hsq 0, effects 0.0 and lod 0.0.
// sigma2 is the residual variance on the whitened scale, the s2 of §32's model.

// One workgroup per target of the chunk.  column[t] is the target's phenotype among the pc of the null fits' chunk,
// point[t] its grid point.  Steps 1-5 are lmm_point_kernel's, written again with the same sums in the same order - lane-strided
// over the samples, wave_sum_all's butterfly, the factorisation by thread 0 - so the LOD is gbrs_scan_lmm_run's at (column,
// point) bit for bit.  w is the workgroup's LDS (ws null) or its own HP n_ld doubles of ws; the sums and their order are the
// same either way.  The dense part runs in LDS in a fixed order: thread j < H - 1 forms column j of R by forward substitution
// down the kept rows, thread 0 closes R, builds and factors C and solves for C^-1 a, thread h < H solves for C^-1 R[:, h] and
// writes effect and se of founder h.  Nothing a target reads or writes depends on another target or on its place.
template <int HP>
__global__ void __launch_bounds__(SC_THREADS)
lmm_effects_kernel(int n, int H, int cz, int64_t n_ld, int n_eig, double half_n, const int32_t *__restrict__ eig_of_point,
                   const double *__restrict__ R, const double *__restrict__ sw_all, const double *__restrict__ qz_all,
                   const double *__restrict__ yt_all, const double *__restrict__ rss0, const double *__restrict__ hsq,
                   const int64_t *__restrict__ column, const int64_t *__restrict__ point, double *__restrict__ ws,
                   double *__restrict__ effect, double *__restrict__ se, double *__restrict__ lod, double *__restrict__ sigma2,
                   int32_t *__restrict__ rank, double *__restrict__ hsq_out) {
    constexpr int HF = HP + 1;                 // founders at most
    extern __shared__ double lmm_eff_dyn[];
    __shared__ double qtx[LM_MAX_C * HP];
    __shared__ double G[HP * HP], L[HP * HP], raw[HP], b[HP];
    __shared__ double Rm[HP * HF], Lc[HP * HP], z[HP], u[HF * HP], sd[1];
    __shared__ int keep[HP], rows[HP], kept_n[1];
    const int64_t t = blockIdx.x, m = point[t], p = column[t];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, Hx = H - 1, e = eig_of_point[m];
    double *w = ws ? ws + t * HP * n_ld : lmm_eff_dyn;
    const double *r = R + m * HP * n_ld;
    const int64_t pe = p * n_eig + e;
    const double *sw = sw_all + pe * n_ld, *qz = qz_all + pe * cz * n_ld, *yt = yt_all + pe * n_ld;
    for (int idx = tid; idx < n * Hx; idx += SC_THREADS) {
        const int j = idx / n, s = idx % n;
        w[j * n_ld + s] = sw[s] * r[j * n_ld + s];
    }
    __syncthreads();
    for (int q = wave; q < (cz + 1) * Hx; q += SC_THREADS / 64) {
        const int k = q / Hx, j = q % Hx;
        double acc = 0.0;
        if (k < cz)
            for (int s = lane; s < n; s += 64) acc += qz[k * n_ld + s] * w[j * n_ld + s];
        else
            for (int s = lane; s < n; s += 64) acc += w[j * n_ld + s] * w[j * n_ld + s];
        acc = wave_sum_all(acc);
        if (lane == 0) (k < cz ? qtx[k * HP + j] : raw[j]) = acc;
    }
    __syncthreads();
    for (int idx = tid; idx < n * Hx; idx += SC_THREADS) {
        const int j = idx / n, s = idx % n;
        double proj = 0.0;
        for (int k = 0; k < cz; ++k) proj += qz[k * n_ld + s] * qtx[k * HP + j];
        w[j * n_ld + s] -= proj;
    }
    __syncthreads();
    const int pairs = Hx * (Hx + 1) / 2;
    for (int q = wave; q < pairs + Hx; q += SC_THREADS / 64) {
        double acc = 0.0;
        if (q < pairs) {
            int j = 0;
            while ((j + 1) * (j + 2) / 2 <= q) ++j;
            const int i = q - j * (j + 1) / 2;
            for (int s = lane; s < n; s += 64) acc += w[j * n_ld + s] * w[i * n_ld + s];
            acc = wave_sum_all(acc);
            if (lane == 0) G[j * HP + i] = acc;
        } else {
            const int j = q - pairs;
            for (int s = lane; s < n; s += 64) acc += w[j * n_ld + s] * yt[s];
            acc = wave_sum_all(acc);
            if (lane == 0) b[j] = acc;
        }
    }
    __syncthreads();
    if (tid == 0) {
        int kept = 0;
        double ess = 0.0;
        for (int j = 0; j < Hx; ++j) {
            const double gjj = G[j * HP + j];
            double d = gjj, zz = b[j];
            for (int i = 0; i < j; ++i) {
                double v = 0.0;
                if (keep[i]) {
                    v = G[j * HP + i];
                    for (int k = 0; k < i; ++k)
                        if (keep[k]) v -= L[j * HP + k] * L[i * HP + k];
                    v /= L[i * HP + i];
                    d -= v * v;
                    zz -= v * b[i];         // b[i] holds a_i by now
                }
                L[j * HP + i] = v;
            }
            const int ok = gjj > SC_PIVOT * raw[j] && d > SC_PIVOT * gjj;
            keep[j] = ok;
            if (ok) {
                rows[kept++] = j;
                L[j * HP + j] = sqrt(d);
                b[j] = zz / L[j * HP + j];
                ess += b[j] * b[j];
            } else {
                for (int i = 0; i <= j; ++i) L[j * HP + i] = 0.0;
                b[j] = 0.0;
            }
        }
        kept_n[0] = kept;
        const double rss = rss0[pe];
        const double rss1 = rss - ess > 0.0 ? rss - ess : 0.0;
        const double s2 = rss1 / (double)(n - cz - kept);
        sd[0] = sqrt(s2);
        lod[t] = scan_lod(rss, ess, half_n);
        sigma2[t] = s2;
        rank[t] = kept;
        hsq_out[t] = hsq[pe];
    }
    __syncthreads();
    const int rk = kept_n[0];
    // column j of R = L_S^-1 G[S, j]: G is kept as its lower triangle
    if (tid < Hx) {
        const int j = tid;
        for (int pp = 0; pp < rk; ++pp) {
            const int i = rows[pp];
            double v = i >= j ? G[i * HP + j] : G[j * HP + i];
            for (int q = 0; q < pp; ++q) v -= L[i * HP + rows[q]] * Rm[q * HF + j];
            Rm[pp * HF + j] = v / L[i * HP + i];
        }
    }
    __syncthreads();
    if (tid == 0) {
        for (int pp = 0; pp < rk; ++pp) {
            double last = 0.0;
            for (int j = 0; j < Hx; ++j) last += Rm[pp * HF + j];
            Rm[pp * HF + Hx] = -last;
        }
        // C = R R' and its Cholesky factor, row by row
        for (int pp = 0; pp < rk; ++pp)
            for (int q = 0; q <= pp; ++q) {
                double v = 0.0;
                for (int h = 0; h < H; ++h) v += Rm[pp * HF + h] * Rm[q * HF + h];
                for (int k = 0; k < q; ++k) v -= Lc[pp * HP + k] * Lc[q * HP + k];
                Lc[pp * HP + q] = pp == q ? sqrt(v) : v / Lc[q * HP + q];
            }
        // z = C^-1 a: forward, then backward
        for (int pp = 0; pp < rk; ++pp) {
            double v = b[rows[pp]];
            for (int k = 0; k < pp; ++k) v -= Lc[pp * HP + k] * z[k];
            z[pp] = v / Lc[pp * HP + pp];
        }
        for (int pp = rk - 1; pp >= 0; --pp) {
            double v = z[pp];
            for (int k = pp + 1; k < rk; ++k) v -= Lc[k * HP + pp] * z[k];
            z[pp] = v / Lc[pp * HP + pp];
        }
    }
    __syncthreads();
    if (tid < H) {
        const int h = tid;
        double *v = u + h * HP, ef = 0.0, norm = 0.0;
        for (int pp = 0; pp < rk; ++pp) {
            double x = Rm[pp * HF + h];
            for (int k = 0; k < pp; ++k) x -= Lc[pp * HP + k] * v[k];
            v[pp] = x / Lc[pp * HP + pp];
        }
        for (int pp = rk - 1; pp >= 0; --pp) {
            double x = v[pp];
            for (int k = pp + 1; k < rk; ++k) x -= Lc[k * HP + pp] * v[k];
            v[pp] = x / Lc[pp * HP + pp];
        }
        for (int pp = 0; pp < rk; ++pp) {
            ef += Rm[pp * HF + h] * z[pp];
            norm += v[pp] * v[pp];
        }
        effect[t * H + h] = ef;
        se[t * H + h] = sd[0] * sqrt(norm);
    }
}
