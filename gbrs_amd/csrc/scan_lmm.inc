// Linear mixed model with LOCO kinship on the scan handle (gbrs_scan_kinship, gbrs_scan_lmm_prepare, gbrs_scan_lmm_run;
// DESIGN.md §32).  Included by scan.hip inside namespace gbrs.
//
// The polygenic effect's covariance is h K + (1 - h) I with K the kinship of the chromosomes other than the scanned one.
// The host factors K = U diag(lambda) U'; in the basis U the covariance is diagonal, so the model is §27's regression
// with one weight per rotated sample.  Four kernels:
//   lmm_kinship_kernel  S_c = A_c A_c' per chromosome, A_c the cohort's dosages on c as [n][M_c H]
//   lmm_rotate_kernel   C = U' B for the dosages (into [M][Hp][n_ld]), the covariates and the phenotypes
//   lmm_null_kernel     per (phenotype, decomposition): the REML search of h, then the weights' square roots, the
//                       weighted covariates' orthonormal basis and the projected weighted phenotype
//   lmm_point_kernel    per (grid point, phenotype): §27's steps 2-5 on the weighted columns, b = X~' y~ and one
//                       forward substitution; LODs only
// The rule every sum follows is scan_prepare_kernel's: one wavefront, lane l adds the samples l, l + 64, ... in order, the
// 64 partial sums meet in a butterfly.  Nothing looks at where a phenotype sits in its chunk or how the cohort was appended.

constexpr int LM_MAX_C = 16;               // covariate columns of the mixed model, intercept included
constexpr int LM_MAX_N = 4096;             // samples: n_eig matrices of n x n doubles stay on the device
constexpr int LM_GRID = 20, LM_GOLDEN = 48;
constexpr double LM_LAMBDA = 1e-10;        // every eigenvalue must exceed this share of the largest
constexpr int LM_TILE = 64;                // phenotypes a workgroup of lmm_point_kernel walks at one grid point
constexpr size_t LM_LDS_BYTES = 48 << 10;  // a point's weighted columns [HP][n_ld] stay in LDS up to this size
constexpr size_t LM_WS_BYTES = (size_t)512 << 20;      // else in a workspace of at most this size, the points in batches

// ---- kinship -----------------------------------------------------------------------------------------------------------------

// match_fetch / match_put of hmm_match.inc on scan.hip's tile constants: one 64 x SC_KC operand block on its way to LDS.
// VEC2: ld and the chunk's first column are even, every pair of columns is one aligned 16-byte load.  TAIL: the columns
// from `valid` on are zeros and are not read.
template <bool VEC2, bool TAIL>
__device__ __forceinline__ void lmm_fetch(double (&v)[SC_PER], const double *__restrict__ src, int64_t ld, int first, int n_rows,
                                          int valid) {
    const int t = threadIdx.x;
    if constexpr (VEC2 && !TAIL) {
#pragma unroll
        for (int i = 0; i < SC_PER / 2; ++i) {
            const int idx = t + SC_THREADS * i, r = idx / (SC_KC / 2), k = 2 * (idx % (SC_KC / 2));
            const double2 x = *reinterpret_cast<const double2 *>(src + (int64_t)min(first + r, n_rows - 1) * ld + k);
            v[2 * i] = x.x;
            v[2 * i + 1] = x.y;
        }
    } else {
#pragma unroll
        for (int i = 0; i < SC_PER; ++i) {
            const int idx = t + SC_THREADS * i, r = idx / SC_KC, k = idx % SC_KC;
            const double *row = src + (int64_t)min(first + r, n_rows - 1) * ld;
            if constexpr (TAIL) v[i] = k < valid ? row[k] : 0.0;
            else v[i] = row[k];
        }
    }
}

template <bool VEC2>
__device__ __forceinline__ void lmm_put(double *dst, const double (&v)[SC_PER]) {
    const int t = threadIdx.x;
    if constexpr (VEC2) {
#pragma unroll
        for (int i = 0; i < SC_PER / 2; ++i) {
            const int idx = t + SC_THREADS * i, r = idx / (SC_KC / 2), k = 2 * (idx % (SC_KC / 2));
            *reinterpret_cast<double2 *>(dst + r * SC_LD + k) = double2{v[2 * i], v[2 * i + 1]};
        }
    } else {
#pragma unroll
        for (int i = 0; i < SC_PER; ++i) {
            const int idx = t + SC_THREADS * i;
            dst[(idx / SC_KC) * SC_LD + idx % SC_KC] = v[i];
        }
    }
}

// blockIdx.x, blockIdx.y: blocks of 64 samples (rows and columns of S_c), blockIdx.z: chromosome.  Both operands are rows
// of the cohort, chromosome c their columns [point_off[c] H, point_off[c + 1] H): match_cross_kernel with a = b.  One chain
// of MFMAs per entry walks the K chunks in order, the K tail is one more chunk staged with zero fill; no atomics, K is not
// split.  Entry (a, b) and entry (b, a) multiply the same pairs in the same order.  A chromosome without points gives
// zeros.  S is [n_chrom][n][n].
template <bool VEC2>
__global__ void __launch_bounds__(SC_THREADS)
lmm_kinship_kernel(int n, int H, int64_t ld, const int64_t *__restrict__ point_off, const double *__restrict__ D,
                   double *__restrict__ S) {
    __shared__ __attribute__((aligned(16))) double lds_a[SC_ROWS * SC_LD];
    __shared__ __attribute__((aligned(16))) double lds_b[SC_COLS * SC_LD];
    const int c = blockIdx.z;
    const int64_t k_off = point_off[c] * H, k_len = (point_off[c + 1] - point_off[c]) * H;
    const int row0 = blockIdx.x * SC_ROWS, col0 = blockIdx.y * SC_COLS;
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
    const double *pa = D + k_off;
    const int64_t chunks = k_len / SC_KC;
    double va[SC_PER], vb[SC_PER];
    if (chunks > 0) {
        lmm_fetch<VEC2, false>(va, pa, ld, row0, n, 0);
        lmm_fetch<VEC2, false>(vb, pa, ld, col0, n, 0);
        for (int64_t m = 1; m < chunks; ++m) {
            lmm_put<VEC2>(lds_a, va);
            lmm_put<VEC2>(lds_b, vb);
            __syncthreads();
            lmm_fetch<VEC2, false>(va, pa + m * SC_KC, ld, row0, n, 0);
            lmm_fetch<VEC2, false>(vb, pa + m * SC_KC, ld, col0, n, 0);
            multiply();
            __syncthreads();
        }
        lmm_put<VEC2>(lds_a, va);
        lmm_put<VEC2>(lds_b, vb);
        __syncthreads();
        multiply();
        __syncthreads();
    }
    const int tail = (int)(k_len - chunks * SC_KC);
    if (tail) {
        lmm_fetch<false, true>(va, pa + chunks * SC_KC, ld, row0, n, tail);
        lmm_fetch<false, true>(vb, pa + chunks * SC_KC, ld, col0, n, tail);
        lmm_put<false>(lds_a, va);
        lmm_put<false>(lds_b, vb);
        __syncthreads();
        multiply();
    }
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = row0 + wave * 16 + g + 4 * r, col = col0 + t * 16 + i;
            if (row < n && col < n) S[((int64_t)c * n + row) * n + col] = acc[t][r];
        }
}

// K[a][b] = scale * (sum over the chromosomes c != leave_out of S_c[a][b], in chromosome order) / count.
__global__ void __launch_bounds__(256)
lmm_kinship_sum_kernel(int64_t nn, int n_chrom, int leave_out, double scale, double count, const double *__restrict__ S,
                       double *__restrict__ K) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= nn) return;
    double acc = 0.0;
    for (int c = 0; c < n_chrom; ++c)
        if (c != leave_out) acc += S[c * nn + idx];
    K[idx] = scale * acc / count;
}

// ---- rotation ----------------------------------------------------------------------------------------------------------------

// out[r][i] = sum over the samples s of src[s][r] U[s][i]: C = U' B, stored transposed so that the rotated sample axis
// is contiguous (out is [rows][n_ld], zeros from column n on).  B is row-major with the samples strided: row r of the
// output is the source column (r / HP) hs + r % HP, present when r % HP < keep (the dosages: HP the padded founder count,
// keep = H - 1, hs = H, so the rows come out as scan_prepare_kernel's [M][HP][n_ld] with zero padding rows; a table of
// columns: HP = keep = hs = 1).  blockIdx.x: block of 64 rows, blockIdx.y: block of 64 rotated samples.  A K chunk of 32
// samples goes through LDS with the sample index outermost for both operands - B's loads run along its rows, U's along its
// rows - so the chunk is transposed on its way to the MFMA operands: lane (i, g) reads [kk + g][16 w + i], 16 consecutive
// doubles per g and LR_LD = 80 doubles (32 banks) between the two g of a half wavefront.  v_mfma_f64_16x16x4_f64, one chain
// per entry over the chunks in order; K is not split.  Every staging load is predicated: n need not be a multiple of 32.
constexpr int LR_LD = 64 + 16;
static_assert((2 * LR_LD) % 64 == 32, "the two sample rows of a half wavefront fall on different banks");

__global__ void __launch_bounds__(SC_THREADS)
lmm_rotate_kernel(int n, int64_t n_ld, int64_t rows, int HP, int keep, int64_t hs, int64_t ld_s, const double *__restrict__ U,
                  const double *__restrict__ src, double *__restrict__ out) {
    __shared__ double lds_a[SC_KC * LR_LD];
    __shared__ double lds_b[SC_KC * LR_LD];
    const int64_t row0 = (int64_t)blockIdx.x * 64, col0 = (int64_t)blockIdx.y * 64;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, i = lane & 15, g = lane >> 4;
    scan_d4 acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = scan_d4{0.0, 0.0, 0.0, 0.0};
    const int r = threadIdx.x & 63, k_first = threadIdx.x >> 6;
    const int64_t row = row0 + r, col = col0 + r;
    const bool row_on = row < rows && row % HP < keep, col_on = col < n;
    const int64_t src_col = row / HP * hs + row % HP;
    for (int k0 = 0; k0 < n; k0 += SC_KC) {
#pragma unroll
        for (int u = 0; u < SC_KC / 4; ++u) {
            const int k = k_first + 4 * u, s = k0 + k;
            lds_a[k * LR_LD + r] = row_on && s < n ? src[(int64_t)s * ld_s + src_col] : 0.0;
            lds_b[k * LR_LD + r] = col_on && s < n ? U[(int64_t)s * n + col] : 0.0;
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < SC_KC; kk += 4) {
            const double av = lds_a[(kk + g) * LR_LD + wave * 16 + i];
#pragma unroll
            for (int t = 0; t < 4; ++t)
                acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, lds_b[(kk + g) * LR_LD + t * 16 + i], acc[t], 0, 0, 0);
        }
        __syncthreads();
    }
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int64_t orow = row0 + wave * 16 + g + 4 * q, ocol = col0 + t * 16 + i;
            if (orow < rows && ocol < n_ld) out[orow * n_ld + ocol] = acc[t][q];
        }
}

// ---- null fit ----------------------------------------------------------------------------------------------------------------

// f(h) = (n - cz) log rss + sum log v_i + log det A of one phenotype in one rotation (REML), +inf where rss <= 0 or A is
// not positive definite.  One wavefront: the weights 1 / v_i go to om (each lane writes and reads its own samples), the
// sums of A = Z*' O Z*, b = Z*' O y* and y*' O y* are lane-strided with the butterfly, lane 0 factors A and everybody
// reads the two results back.  sh: cz (cz + 1) / 2 + cz + 4 doubles of LDS.
__device__ double lmm_reml(int n, int cz, double h, const double *__restrict__ ys, const double *__restrict__ zs, int64_t n_ld,
                           const double *__restrict__ lam, double *__restrict__ om, double *sh, double *rss_out) {
    const int lane = threadIdx.x;
    double *A = sh, *b = sh + LM_MAX_C * LM_MAX_C, *res = b + LM_MAX_C;
    double lv = 0.0, yy = 0.0;
    for (int s = lane; s < n; s += 64) {
        const double v = h * lam[s] + (1.0 - h);
        om[s] = 1.0 / v;
        lv += log(v);
    }
    lv = wave_sum_all(lv);
    for (int j = 0; j < cz; ++j) {
        for (int i = 0; i <= j; ++i) {
            double acc = 0.0;
            for (int s = lane; s < n; s += 64) acc += zs[j * n_ld + s] * (om[s] * zs[i * n_ld + s]);
            acc = wave_sum_all(acc);
            if (lane == 0) A[j * LM_MAX_C + i] = acc;
        }
        double acc = 0.0;
        for (int s = lane; s < n; s += 64) acc += zs[j * n_ld + s] * (om[s] * ys[s]);
        acc = wave_sum_all(acc);
        if (lane == 0) b[j] = acc;
    }
    for (int s = lane; s < n; s += 64) yy += (om[s] * ys[s]) * ys[s];
    yy = wave_sum_all(yy);
    __syncthreads();
    if (lane == 0) {
        bool pd = true;
        double logdet = 0.0, tt = 0.0;
        for (int j = 0; j < cz && pd; ++j) {            // A = L L' in place, t = L^-1 b in place
            double t = b[j];
            for (int i = 0; i < j; ++i) {
                double v = A[j * LM_MAX_C + i];
                for (int k = 0; k < i; ++k) v -= A[j * LM_MAX_C + k] * A[i * LM_MAX_C + k];
                v /= A[i * LM_MAX_C + i];
                A[j * LM_MAX_C + i] = v;
                t -= v * b[i];
            }
            double d = A[j * LM_MAX_C + j];
            for (int k = 0; k < j; ++k) d -= A[j * LM_MAX_C + k] * A[j * LM_MAX_C + k];
            pd = d > 0.0;
            if (pd) {
                d = sqrt(d);
                A[j * LM_MAX_C + j] = d;
                b[j] = t / d;
                tt += b[j] * b[j];
                logdet += log(d);
            }
        }
        const double rss = yy - tt;
        res[0] = pd && rss > 0.0 ? (n - cz) * log(rss) + lv + 2.0 * logdet : __builtin_huge_val();
        res[1] = rss;
    }
    __syncthreads();
    const double f = res[0];
    *rss_out = res[1];
    __syncthreads();
    return f;
}

// blockIdx.x: phenotype of the chunk, blockIdx.y: decomposition; one wavefront.  ys is [n_eig][pc][n_ld], zs
// [n_eig][cz][n_ld], lam [n_eig][n]; hsq_in [pc][n_eig] or null.  The search (DESIGN.md §32): f on k / 20, k = 0 .. 20, the
// lowest wins and the lowest k among equals; the bracket is its two neighbours clipped to [0, 1]; 48 golden-section steps,
// the left point staying on equal f; the midpoint, unless the bracket still touches 0 or 1 and f there is not above f at
// the midpoint.  rss <= 0 at h = 0 (a column of zeros): hsq 0, sigma2 0, rss0 0, so that every LOD is 0.0.
// Then, at the h found: sw = v^-1/2 (zeros past sample n), qz = the weighted covariates after modified Gram-Schmidt in
// column order, each column swept twice over the ones before it and then normalised, yt = sw y* - qz qz' (sw y*), rss0 =
// |yt|^2.  Outputs per (p, e): hsq, sigma2 = rss / (n - cz), sw [n_ld], qz [cz][n_ld], yt [n_ld], rss0; the wavefront of
// decomposition 0 also resets the phenotype's rank range for lmm_point_kernel.
__global__ void __launch_bounds__(64)
lmm_null_kernel(int n, int cz, int64_t n_ld, int64_t pc, int n_eig, const double *__restrict__ ys_all, const double *__restrict__ zs_all,
                const double *__restrict__ lam_all, const double *__restrict__ hsq_in, double *__restrict__ hsq,
                double *__restrict__ sigma2, double *__restrict__ sw_all, double *__restrict__ qz_all, double *__restrict__ yt_all,
                double *__restrict__ rss0, int32_t *__restrict__ rank_min, int32_t *__restrict__ rank_max) {
    __shared__ double sh[LM_MAX_C * LM_MAX_C + LM_MAX_C + 4];
    __shared__ double qty[LM_MAX_C];
    const int64_t p = blockIdx.x;
    const int e = blockIdx.y, lane = threadIdx.x;
    const int64_t pe = p * n_eig + e;
    const double *ys = ys_all + ((int64_t)e * pc + p) * n_ld, *zs = zs_all + (int64_t)e * cz * n_ld, *lam = lam_all + (int64_t)e * n;
    double *sw = sw_all + pe * n_ld, *qz = qz_all + pe * cz * n_ld, *yt = yt_all + pe * n_ld;
    if (e == 0 && lane == 0) {
        rank_min[p] = 0x7fffffff;
        rank_max[p] = 0;
    }
    double rss = 0.0, h = 0.0;
    auto f = [&](double at) { return lmm_reml(n, cz, at, ys, zs, n_ld, lam, sw, sh, &rss); };
    const double f0 = f(0.0);
    const bool flat = rss <= 0.0;
    if (!flat && hsq_in) h = hsq_in[pe];
    if (!flat && !hsq_in) {
        double fbest = f0, f1 = f0;
        int best = 0;
        for (int k = 1; k <= LM_GRID; ++k) {
            f1 = f((double)k / LM_GRID);
            if (f1 < fbest) {
                fbest = f1;
                best = k;
            }
        }
        double a = (double)(best > 0 ? best - 1 : 0) / LM_GRID, b = (double)(best < LM_GRID ? best + 1 : LM_GRID) / LM_GRID;
        const double invphi = (sqrt(5.0) - 1.0) / 2.0;
        double c = b - invphi * (b - a), d = a + invphi * (b - a);
        double fc = f(c), fd = f(d);
        for (int step = 0; step < LM_GOLDEN; ++step) {
            if (fc <= fd) {
                b = d;
                d = c;
                fd = fc;
                c = b - invphi * (b - a);
                fc = f(c);
            } else {
                a = c;
                c = d;
                fc = fd;
                d = a + invphi * (b - a);
                fd = f(d);
            }
        }
        h = 0.5 * (a + b);
        double fh = f(h);
        if (a == 0.0 && f0 <= fh) {
            h = 0.0;
            fh = f0;
        }
        if (b == 1.0 && f1 <= fh) h = 1.0;
    }
    if (!flat) (void)f(h);              // rss at the h that stands
    // the weights' square roots
    for (int64_t s = lane; s < n_ld; s += 64) sw[s] = s < n ? sqrt(1.0 / (h * lam[s] + (1.0 - h))) : 0.0;
    // the basis of the weighted covariates
    for (int j = 0; j < cz; ++j) {
        double *qj = qz + j * n_ld;
        for (int64_t s = lane; s < n_ld; s += 64) qj[s] = s < n ? sw[s] * zs[j * n_ld + s] : 0.0;
        for (int sweep = 0; sweep < 2; ++sweep)
            for (int k = 0; k < j; ++k) {
                const double *qk = qz + k * n_ld;
                double dot = 0.0;
                for (int s = lane; s < n; s += 64) dot += qk[s] * qj[s];
                dot = wave_sum_all(dot);
                for (int s = lane; s < n; s += 64) qj[s] -= dot * qk[s];
            }
        double nrm = 0.0;
        for (int s = lane; s < n; s += 64) nrm += qj[s] * qj[s];
        nrm = sqrt(wave_sum_all(nrm));
        for (int s = lane; s < n; s += 64) qj[s] /= nrm;
    }
    // the projected weighted phenotype
    for (int k = 0; k < cz; ++k) {
        double acc = 0.0;
        for (int s = lane; s < n; s += 64) acc += qz[k * n_ld + s] * (sw[s] * ys[s]);
        acc = wave_sum_all(acc);
        if (lane == 0) qty[k] = acc;
    }
    __syncthreads();
    double ss = 0.0;
    for (int64_t s = lane; s < n_ld; s += 64) {
        double v = 0.0;
        if (s < n) {
            double proj = 0.0;
            for (int k = 0; k < cz; ++k) proj += qz[k * n_ld + s] * qty[k];
            v = sw[s] * ys[s] - proj;
        }
        yt[s] = v;
        ss += v * v;
    }
    ss = wave_sum_all(ss);
    if (lane == 0) {
        hsq[pe] = h;
        sigma2[pe] = flat ? 0.0 : rss / (n - cz);
        rss0[pe] = flat ? 0.0 : ss;
    }
}

// ---- the weighted scan ---------------------------------------------------------------------------------------------------------

// blockIdx.x: grid point m0 + blockIdx.x, blockIdx.y: tile of `tile` phenotypes of the chunk, walked one after the other;
// the rotated columns R_m [HP][n_ld] are read once per phenotype and come from L2 after the first.  Per phenotype, with e
// the point's decomposition and scan_prepare_kernel's sums and its factorisation by one thread:
//   1  w[j][s] = sw[s] R_m[j][s] for the H - 1 kept founders
//   2  qtx[k][j] = sum_s qz[k][s] w[j][s], raw[j] = sum_s w[j][s]^2
//   3  w[j][s] -= sum_k qz[k][s] qtx[k][j]
//   4  G[j][i] = sum_s w[j][s] w[i][s], i <= j;  b[j] = sum_s w[j][s] yt[s]
//   5  Cholesky with the skip rule (SC_PIVOT, and G_jj <= SC_PIVOT raw[j] counts as G_jj = 0), z = L^-1 b down the kept
//      columns, ess = |z|^2, the LOD by scan_lod into the chunk's [P][M] rows
// No W is written.  w is the workgroup's LDS (ws null) or its own HP n_ld doubles of ws; the sums and their order are the
// same either way.  The phenotype's rank range takes the point's rank by integer atomics.
// lmm_effects_kernel (scan_lmm_effects.inc) repeats steps 1-5 line for line so that its LOD carries this kernel's bits: a
// change of a sum, of its order or of the factorisation here must be made there too (test_scan_lmm_effects_gpu.py compares with ==).
template <int HP>
__global__ void __launch_bounds__(SC_THREADS)
lmm_point_kernel(int n, int64_t M, int64_t m0, int H, int cz, int64_t n_ld, int64_t pc, int n_eig, int tile, double half_n,
                 const int32_t *__restrict__ eig_of_point, const double *__restrict__ R, const double *__restrict__ sw_all,
                 const double *__restrict__ qz_all, const double *__restrict__ yt_all, const double *__restrict__ rss0,
                 double *__restrict__ ws, double *__restrict__ lod, int32_t *__restrict__ rank_min, int32_t *__restrict__ rank_max) {
    extern __shared__ double lmm_dyn[];
    __shared__ double qtx[LM_MAX_C * HP];
    __shared__ double G[HP * HP], L[HP * HP], raw[HP], b[HP];
    __shared__ int keep[HP];
    const int64_t m = m0 + blockIdx.x;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, Hx = H - 1, e = eig_of_point[m];
    double *w = ws ? ws + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * HP * n_ld : lmm_dyn;
    const double *r = R + m * HP * n_ld;
    const int64_t p_end = min((int64_t)(blockIdx.y + 1) * tile, pc);
    for (int64_t p = (int64_t)blockIdx.y * tile; p < p_end; ++p) {
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
                double d = gjj, z = b[j];
                for (int i = 0; i < j; ++i) {
                    double v = 0.0;
                    if (keep[i]) {
                        v = G[j * HP + i];
                        for (int k = 0; k < i; ++k)
                            if (keep[k]) v -= L[j * HP + k] * L[i * HP + k];
                        v /= L[i * HP + i];
                        d -= v * v;
                        z -= v * b[i];          // b[i] holds z_i by now
                    }
                    L[j * HP + i] = v;
                }
                const int ok = gjj > SC_PIVOT * raw[j] && d > SC_PIVOT * gjj;
                keep[j] = ok;
                kept += ok;
                if (ok) {
                    L[j * HP + j] = sqrt(d);
                    b[j] = z / L[j * HP + j];
                    ess += b[j] * b[j];
                } else {
                    for (int i = 0; i <= j; ++i) L[j * HP + i] = 0.0;
                    b[j] = 0.0;
                }
            }
            lod[p * M + m] = scan_lod(rss0[pe], ess, half_n);
            atomicMin(&rank_min[p], kept);
            atomicMax(&rank_max[p], kept);
        }
        __syncthreads();
    }
}
