// Mediation of QTL peaks on the scan handle (gbrs_scan_mediate; DESIGN.md §30).  Included by scan.hip inside namespace
// gbrs, after the product kernel's helpers.  For a target t - a phenotype column y_t and a grid point m = point[t] - every
// mediator column z_q joins the covariates in turn and the LOD of y_t at m is formed again; W_m = L^-1 X~' of
// gbrs_scan_prepare serves every pair, no new factorisation.  No fused multiply-add anywhere (-ffp-contract=off).
//
// The rule.  y~_t and z~_q are the projections v - qz qz' v by scan_pheno_kernel, which also gives s_yy = |y~_t|^2 and
// s_zz = |z~_q|^2.  Per (t, q):
//   a = W_m y~_t           b = W_m z~_q          s_yz = y~_t . z~_q
//   rss1 = s_yy - |a|^2                          lod0[t] = scan_lod(s_yy, |a|^2, n / 2)
//   e_zz = s_zz - |b|^2    e_yz = s_yz - a . b
//   rss0' = s_yy - s_yz^2 / s_zz                 (the target given covariates + mediator)
//   rss1' = rss1 - e_yz^2 / e_zz                 (given covariates + mediator + founders at m)
//   lod_med = (n / 2) log10(rss0' / rss1'), 0.0 where rss0' == 0, +inf where rss1' <= 0 < rss0'
// The pair is unused (used = 0, lod_med = NaN) when
//   s_zz == 0                  the mediator lies in the covariates' span
//   e_zz <= SC_PIVOT s_zz      the mediator lies in the span of covariates + founders at m
//   rss0' <= SC_PIVOT s_yy     the target lies in the span of covariates + mediator (q = the target itself)
// Per target over its used mediators: n_used, mean and sd (two passes, n_used - 1 in the denominator, NaN below 2) and the
// K used mediators with the lowest lod_med in ascending (lod_med, index) order, -1 / NaN in the missing places.

constexpr int64_t SM_TCHUNK = 512;           // targets whose [Tc][Q] LODs are on the device at a time
constexpr int SM_MAX_K = 64;                 // places of the top list
static_assert(SM_TCHUNK % (SC_ROWS / 8) == 0 && SM_TCHUNK % (SC_ROWS / 16) == 0,
              "a chunk is whole row tiles, so a target's place in its tile does not depend on the chunk");

// One wavefront per target of the chunk: a[j] = W_m[j] . y~_t for the HP rows of the target's point, lane l adding the
// samples l, l + 64, ... in order and the partial sums meeting in the butterfly (the zeros past sample n add nothing);
// |a|^2 in row order; rss1 and lod0.
template <int HP>
__global__ void __launch_bounds__(64)
scan_med_target_kernel(int64_t n_ld, double half_n, const double *__restrict__ W, const int64_t *__restrict__ point,
                       const double *__restrict__ yt, const double *__restrict__ syy, double *__restrict__ a,
                       double *__restrict__ rss1, double *__restrict__ lod0) {
    const int64_t t = blockIdx.x;
    const int lane = threadIdx.x;
    const double *w = W + point[t] * HP * n_ld, *y = yt + t * n_ld;
    double ess = 0.0;
    for (int j = 0; j < HP; ++j) {
        double acc = 0.0;
        for (int64_t s = lane; s < n_ld; s += 64) acc += w[j * n_ld + s] * y[s];
        acc = wave_sum_all(acc);
        if (lane == 0) a[t * HP + j] = acc;
        ess += acc * acc;
    }
    if (lane == 0) {
        rss1[t] = syy[t] - ess;
        lod0[t] = scan_lod(syy[t], ess, half_n);
    }
}

// The rule for one pair from its six numbers; returns used.
__device__ __forceinline__ bool scan_med_rule(double syy, double rss1, double szz, double syz, double bb, double ab, double half_n,
                                              double *lod) {
    *lod = __builtin_nan("");
    if (szz == 0.0) return false;
    const double ezz = szz - bb;
    if (ezz <= SC_PIVOT * szz) return false;
    const double rss0p = syy - syz * syz / szz;
    if (rss0p <= SC_PIVOT * syy) return false;
    const double eyz = syz - ab;
    const double rss1p = rss1 - eyz * eyz / ezz;
    *lod = rss0p == 0.0 ? 0.0 : rss1p <= 0.0 ? __builtin_huge_val() : half_n * log10(rss0p / rss1p);
    return true;
}

// scan_lod_kernel with gathered rows: blockIdx.x: block of 64 mediators (fastest: the blocks side by side share the
// gathered rows), blockIdx.y: block of 64 / HP targets of the chunk.  Row r of the tile is row r % HP of W at the point
// of target r / HP, its base read from the chunk's point table; several targets may share a point.  The operand maps, the
// LDS stride, the K chunks and the prefetch are scan_lod_kernel's.  s_yz is a second, small product in the same walk
// over the samples: the y~ rows of the tile's targets are a third operand block of 16 rows (those past the tile's
// targets are not used), and wavefront w multiplies it with its own 16 mediators w 16 .. w 16 + 15, one more accumulator
// per wavefront.  K = n_ld is one chain of MFMAs per accumulator, not split and without atomics.
// Epilogue: register r of lane (g, i) of accumulator u is b of row g + 4 r of the wavefront's 16 rows and mediator
// 16 u + i.  |b|^2 and a . b are added in the lane in register order, then across the four lane groups (xor 16, xor 32),
// as scan_lod_kernel adds ess: they depend on nothing but the target's rows and the mediator.  The three numbers go to
// LDS as [target][mediator]; every thread then applies the rule to 64 / HP / 4 pairs and stores lod_med and used,
// consecutive threads consecutive mediators of one target's row.  W z~ never reaches memory.  Targets past Tc and
// mediators past Q shadow the last valid one and are not stored.
template <int HP>
__global__ void __launch_bounds__(SC_THREADS)
scan_med_kernel(int64_t Tc, int64_t Q, int64_t n_ld, double half_n, const double *__restrict__ W,
                const int64_t *__restrict__ point, const double *__restrict__ yt, const double *__restrict__ zt,
                const double *__restrict__ syy, const double *__restrict__ rss1, const double *__restrict__ a,
                const double *__restrict__ szz, double *__restrict__ lod, uint8_t *__restrict__ used) {
    constexpr int PTS = SC_ROWS / HP, PPW = 16 / HP;      // targets per workgroup and per wavefront
    constexpr int YROWS = 16;                             // the y~ operand block: one MFMA's rows
    __shared__ __attribute__((aligned(16))) double lds[(SC_ROWS + SC_COLS + YROWS) * SC_LD];
    static_assert(3 * PTS * SC_COLS <= (SC_ROWS + SC_COLS + YROWS) * SC_LD, "the epilogue's three [target][mediator] fit the operands' LDS");
    static_assert(YROWS * SC_KC / 2 == SC_THREADS && PTS <= YROWS, "one 16-byte load per thread for the y~ block");
    double *lds_a = lds, *lds_b = lds + SC_ROWS * SC_LD, *lds_y = lds + (SC_ROWS + SC_COLS) * SC_LD;
    const int64_t col0 = (int64_t)blockIdx.x * SC_COLS, t0 = (int64_t)blockIdx.y * PTS;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, i = lane & 15, g = lane >> 4;
    // what this thread fetches: rows tid / 16 + 16 u of the two 64-row blocks, row tid / 16 of the y~ block
    const int fr = tid / (SC_KC / 2), fk = 2 * (tid % (SC_KC / 2));
    const double *pa[SC_PER / 2], *pb[SC_PER / 2], *py;
#pragma unroll
    for (int u = 0; u < SC_PER / 2; ++u) {
        const int r = fr + (SC_THREADS / (SC_KC / 2)) * u;
        pa[u] = W + (point[std::min<int64_t>(t0 + r / HP, Tc - 1)] * HP + r % HP) * n_ld + fk;
        pb[u] = zt + std::min<int64_t>(col0 + r, Q - 1) * n_ld + fk;
    }
    py = yt + std::min<int64_t>(t0 + fr, Tc - 1) * n_ld + fk;
    double va[SC_PER], vb[SC_PER];
    double2 vy;
    auto fetch = [&](int64_t k0) {
#pragma unroll
        for (int u = 0; u < SC_PER / 2; ++u) {
            const double2 x = *reinterpret_cast<const double2 *>(pa[u] + k0), z = *reinterpret_cast<const double2 *>(pb[u] + k0);
            va[2 * u] = x.x;
            va[2 * u + 1] = x.y;
            vb[2 * u] = z.x;
            vb[2 * u + 1] = z.y;
        }
        vy = *reinterpret_cast<const double2 *>(py + k0);
    };
    auto put = [&]() {
        scan_put(lds_a, va);
        scan_put(lds_b, vb);
        *reinterpret_cast<double2 *>(lds_y + fr * SC_LD + fk) = vy;
    };
    scan_d4 acc[4], accy = scan_d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int u = 0; u < 4; ++u) acc[u] = scan_d4{0.0, 0.0, 0.0, 0.0};
    const double *ra = lds_a + (wave * 16 + i) * SC_LD + g, *rb = lds_b + i * SC_LD + g, *ry = lds_y + i * SC_LD + g;
    const double *rbw = rb + wave * 16 * SC_LD;
    auto multiply = [&]() {
#pragma unroll
        for (int kk = 0; kk < SC_KC; kk += 4) {
            const double av = ra[kk];
#pragma unroll
            for (int u = 0; u < 4; ++u) acc[u] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, rb[u * 16 * SC_LD + kk], acc[u], 0, 0, 0);
            accy = __builtin_amdgcn_mfma_f64_16x16x4f64(ry[kk], rbw[kk], accy, 0, 0, 0);
        }
    };
    const int64_t chunks = n_ld / SC_KC;       // >= 1
    fetch(0);
    for (int64_t k = 1; k < chunks; ++k) {
        put();
        __syncthreads();
        fetch(k * SC_KC);
        multiply();
        __syncthreads();
    }
    put();
    __syncthreads();
    multiply();
    __syncthreads();
    // a of this lane's four rows: row g + 4 r of the wavefront's 16
    double ar[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int row = wave * 16 + g + 4 * r;
        ar[r] = a[std::min<int64_t>(t0 + row / HP, Tc - 1) * HP + row % HP];
    }
    double *e_bb = lds, *e_ab = lds + PTS * SC_COLS, *e_yz = lds + 2 * PTS * SC_COLS;      // [PTS][64] each
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        double bb[PPW], ab[PPW];
        if constexpr (HP == 8) {
            bb[0] = acc[u][0] * acc[u][0] + acc[u][1] * acc[u][1];
            bb[1] = acc[u][2] * acc[u][2] + acc[u][3] * acc[u][3];
            ab[0] = ar[0] * acc[u][0] + ar[1] * acc[u][1];
            ab[1] = ar[2] * acc[u][2] + ar[3] * acc[u][3];
        } else {
            bb[0] = ((acc[u][0] * acc[u][0] + acc[u][1] * acc[u][1]) + acc[u][2] * acc[u][2]) + acc[u][3] * acc[u][3];
            ab[0] = ((ar[0] * acc[u][0] + ar[1] * acc[u][1]) + ar[2] * acc[u][2]) + ar[3] * acc[u][3];
        }
#pragma unroll
        for (int q = 0; q < PPW; ++q) {
            bb[q] += __shfl_xor(bb[q], 16, WAVE);
            bb[q] += __shfl_xor(bb[q], 32, WAVE);
            ab[q] += __shfl_xor(ab[q], 16, WAVE);
            ab[q] += __shfl_xor(ab[q], 32, WAVE);
            if (g == 0) {
                e_bb[(wave * PPW + q) * SC_COLS + u * 16 + i] = bb[q];
                e_ab[(wave * PPW + q) * SC_COLS + u * 16 + i] = ab[q];
            }
        }
    }
    // s_yz: register r of lane (g, i) is target g + 4 r of the tile, mediator 16 wave + i
#pragma unroll
    for (int r = 0; r < 4; ++r)
        if (g + 4 * r < PTS) e_yz[(g + 4 * r) * SC_COLS + wave * 16 + i] = accy[r];
    __syncthreads();
#pragma unroll
    for (int u = 0; u < SC_COLS * PTS / SC_THREADS; ++u) {
        const int idx = tid + SC_THREADS * u, tl = idx / SC_COLS, col = idx % SC_COLS;
        const int64_t t = t0 + tl, q = col0 + col;
        if (t < Tc && q < Q) {
            double v;
            const bool ok = scan_med_rule(syy[t], rss1[t], szz[q], e_yz[idx], e_bb[idx], e_ab[idx], half_n, &v);
            lod[t * Q + q] = v;
            used[t * Q + q] = ok ? 1 : 0;
        }
    }
}

// One wavefront per target of the chunk over its row of lod_med / used.  Lane l looks at the mediators l, l + 64, ... in
// order; an unused mediator adds nothing, so the order of the sums depends on Q alone.  n_used; the sum and then the
// squared deviations from the mean, each meeting in the butterfly; the K lowest one after the other: every lane keeps the
// lowest (value, index) of its mediators above the place before, and the 64 candidates meet in a butterfly that prefers
// the lower value and, among equal ones, the lower index.  No atomics.
__global__ void __launch_bounds__(64)
scan_med_select_kernel(int64_t Q, int K, const double *__restrict__ lod, const uint8_t *__restrict__ used,
                       double *__restrict__ best_lod, int64_t *__restrict__ best_index, double *__restrict__ mean,
                       double *__restrict__ sd, int64_t *__restrict__ n_used) {
    const int64_t t = blockIdx.x;
    const int lane = threadIdx.x;
    const double *v = lod + t * Q;
    const uint8_t *on = used + t * Q;
    long long count = 0;
    double sum = 0.0;
    for (int64_t q = lane; q < Q; q += 64)
        if (on[q]) {
            ++count;
            sum += v[q];
        }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) count += __shfl_xor(count, off, WAVE);
    sum = wave_sum_all(sum);
    const double mu = count >= 2 ? sum / (double)count : __builtin_nan("");
    double ss = 0.0;
    for (int64_t q = lane; q < Q; q += 64)
        if (on[q]) {
            const double d = v[q] - mu;
            ss += d * d;
        }
    ss = wave_sum_all(ss);
    if (lane == 0) {
        n_used[t] = count;
        mean[t] = mu;
        sd[t] = count >= 2 ? sqrt(ss / (double)(count - 1)) : __builtin_nan("");
    }
    double last = -__builtin_huge_val();
    int64_t last_at = -1;
    for (int k = 0; k < K; ++k) {
        double best = 0.0;
        int64_t at = -1;
        if (k < count)
            for (int64_t q = lane; q < Q; q += 64) {
                if (!on[q]) continue;
                const double x = v[q];
                if (!(x > last || (x == last && q > last_at))) continue;       // at or before the place before
                if (at < 0 || x < best) {
                    best = x;
                    at = q;
                }
            }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const double ov = __shfl_xor(best, off, WAVE);
            const int64_t oa = __shfl_xor((long long)at, off, WAVE);
            if (oa >= 0 && (at < 0 || ov < best || (ov == best && oa < at))) {
                best = ov;
                at = oa;
            }
        }
        if (lane == 0) {
            best_lod[t * K + k] = at < 0 ? __builtin_nan("") : best;
            best_index[t * K + k] = at;
        }
        last = best;
        last_at = at;
    }
}
