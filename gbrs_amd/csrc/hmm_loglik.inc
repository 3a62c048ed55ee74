// Data log-likelihood of the last run (gbrs_hmm_loglik) and of the run's emissions under other transition tables
// (gbrs_hmm_loglik_tables); DESIGN.md §24.  Included by hmm_passes.hip inside namespace gbrs.
//
// With Z_i the normaliser of gene i in the scaled forward recursion documented above forward_viterbi_kernel,
//   log P(data of a chromosome) = sum_i log Z_i.
// The handle's own tables: every forward route (the sequential chains, the two-samples-per-wave chains, the MFMA sweeps
// and the blocked scan, whose chain kernels are the same chain_kernel) leaves 1/Z_i in `invz` as [sample][gene], so
// loglik_reduce_kernel adds up -log(invz) and no recursion runs again.
// Other tables: loglik_tables_kernel runs the forward recursion alone on the emissions the run left in `peprob`, for all
// (candidate table, sample) pairs of one chromosome in one launch, and stores one double per pair.
// Extra device memory: the candidates' log tables as uploaded and exp() of them, transposed per block (exp_blocks_t_kernel):
// n_tables x (n_c - 1) x S^2 x 16 bytes (only the n_c - 1 blocks that are read of a table's n_trans go up), kept on the
// handle and reused by later calls (gbrs_hmm_loglik_info reports what is held).  No environment switch is read here.

// One wavefront per (sample, chromosome): lane l adds up the genes l, l + 64, .. in that order, the 64 partial sums go
// through the xor butterfly.  The shape of the sum depends on the chromosome's length alone, so a value is the same bits
// from run to run, in every slot and batch size.
constexpr int LL_RED_WAVES = 4;
__global__ void __launch_bounds__(64 * LL_RED_WAVES)
loglik_reduce_kernel(int n_chrom, int64_t total_genes, int sample0, const ChromDesc *__restrict__ chroms,
                     const double *__restrict__ invz, double *__restrict__ out /* [n][n_chrom] */) {
    const int lane = threadIdx.x & 63;
    const int c = (int)blockIdx.x * LL_RED_WAVES + (int)(threadIdx.x >> 6);
    if (c >= n_chrom) return;
    const ChromDesc cd = chroms[c];
    const double *iz = invz + (int64_t)(sample0 + (int)blockIdx.y) * total_genes + cd.gene_off;
    double sum = 0.0;
    for (int i = lane; i < cd.n_genes; i += WAVE) sum -= log(iz[i]);
    sum = wave_sum_all(sum);
    if (lane == 0) out[(int64_t)blockIdx.y * n_chrom + c] = sum;
}

// pt[b][k][j] = exp(t[b][j][k]): exp_blocks_kernel's transposed output alone.  The chain's lanes are the target states j,
// so for a source state k they read consecutive doubles.
// `pairs` (S even): two source states side by side, pt[b][k / 2][j][k % 2], so that a lane fetches them in one 16-byte load
// and consecutive lanes read consecutive 16 bytes.
__global__ void exp_blocks_t_kernel(int S, int64_t n_blocks, const double *__restrict__ t, double *__restrict__ pt, bool pairs) {
    const int64_t bs = (int64_t)S * S, total = n_blocks * bs;
    for (int64_t x = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; x < total; x += (int64_t)gridDim.x * blockDim.x) {
        const int64_t b = x / bs;
        const int r = (int)(x - b * bs);
        const int jj = r / S, kk = r % S;
        const int64_t at = pairs ? ((int64_t)(kk >> 1) * S + jj) * 2 + (kk & 1) : (int64_t)kk * S + jj;
        pt[b * bs + at] = exp(t[x]);
    }
}

// value of lane `l` (wavefront-uniform) in every lane, through scalar registers
__device__ __forceinline__ double ll_bcast(double v, int l) {
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), l), __builtin_amdgcn_readlane(__double2loint(v), l));
}

// One wavefront per (candidate table, sample) of one chromosome; lane l carries the states l, l + 64, l + 128 (R of them).
//   gene 0:  y_j = exp(init_j) * pe_0[j]
//   gene i:  x_j = (sum_k y_{i-1}[k] * P[j,k]) / Z_{i-1} + tiny,  y_j = x_j * pe_i[j],  Z_i = sum_j y_j
// The sum over k runs in four interleaved partial sums added as (a0 + a1) + (a2 + a3); y[k] reaches the lanes through
// v_readlane, no LDS.  KCAP > 0 (S <= KCAP <= 64, R = 1): a lane keeps its column of NSET transition blocks in registers,
// the block of step o + NSET being fetched while step o computes, so that no global load sits on the chain.  KCAP = 0:
// any S, the block is streamed through L2 within the step.
// log Z_i: lane i % 64 keeps Z_i, and every 64 genes the lanes take one log each and the 64 values are added in gene order.
// A Z_i that is zero or not finite makes the pair's result -inf.  A state that no path reaches (a zero dot product) gets
// x = tiny even where 1 / Z_{i-1} overflows, as the reference's log(0 + tiny) does.
// SFIX > 0: the state count is this even constant (36, the eight-founder model) and the table is in exp_blocks_t_kernel's
// paired layout: a block's loads take immediate offsets and fetch two entries each, 19 loads per step with the emission's,
// so that the NSET - 1 steps of fetches in flight stay within what a wavefront's load counter can tell apart (63).
template <int R, int KCAP, int NSET, int SFIX = 0>
__global__ void __launch_bounds__(64)
loglik_tables_kernel(int S_arg, int n_genes, int64_t gene_off, int64_t total_genes, int sample0, int n_samples, int n_pairs,
                     const double *__restrict__ pt /* [n_tables][n_genes - 1][S from][S to] */,
                     const double *__restrict__ peprob, const double *__restrict__ init_vec,
                     double *__restrict__ out /* [n_tables][n_samples] */) {
    static_assert(KCAP == 0 || R == 1, "the register-resident columns are for S <= 64");
    static_assert(SFIX == 0 || (SFIX == KCAP && SFIX % 2 == 0), "a fixed state count fills the register-resident column, in pairs");
    const int S = SFIX > 0 ? SFIX : S_arg;
    const int lane = threadIdx.x;
    const int pair = (int)blockIdx.x;
    if (pair >= n_pairs) return;
    const int table = pair / n_samples, slot = pair - table * n_samples;
    const int n_steps = n_genes - 1;
    const int64_t bs = (int64_t)S * S;
    const double *PT = pt + (int64_t)table * n_steps * bs;
    const double *PE = peprob + ((int64_t)(sample0 + slot) * total_genes + gene_off) * S;
    bool act[R];
    int jc[R];                                             // the lane's states, clamped for the loads of idle lanes
#pragma unroll
    for (int r = 0; r < R; ++r) {
        act[r] = r * 64 + lane < S;
        jc[r] = min(r * 64 + lane, S - 1);
    }
    double y[R], z_own = 0.0;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        y[r] = act[r] ? exp(init_vec[jc[r]]) * PE[jc[r]] : 0.0;
        z_own += y[r];
    }
    double z = wave_sum_dpp(z_own);
    double ll = 0.0, z_keep = 1.0;
    bool bad = false;
    auto flush = [&](int count) {                          // the logs of the `count` kept Z, added in gene order
        const double lg = log(z_keep);
        for (int l = 0; l < count; ++l) ll += ll_bcast(lg, l);
    };
    auto keep = [&](int i, double zi) {
        bad = bad || !(zi > 0.0 && zi < INFINITY);
        if (lane == (i & 63)) z_keep = zi;
        if ((i & 63) == 63) flush(64);
    };
    keep(0, z);
    double inv_z = fast_recip_pos(z);

    if constexpr (KCAP > 0) {
        const int last_o = max(n_steps - 1, 0);
        double p[NSET][KCAP], pe[NSET];
        auto fetch = [&](int o, double (&col)[KCAP], double &pe_o) {
            const int oc = min(o, last_o);
            if constexpr (SFIX > 0) {                      // the paired layout: KCAP / 2 loads of 16 bytes
                const double2 *B2 = reinterpret_cast<const double2 *>(PT + (int64_t)oc * bs) + jc[0];
#pragma unroll
                for (int m = 0; m < KCAP / 2; ++m) {
                    const double2 v = B2[m * SFIX];
                    col[2 * m] = v.x;
                    col[2 * m + 1] = v.y;
                }
            } else {
                const double *B = PT + (int64_t)oc * bs + jc[0];
#pragma unroll
                for (int k = 0; k < KCAP; ++k) col[k] = B[(int64_t)min(k, S - 1) * S];
            }
            pe_o = PE[(int64_t)(oc + 1) * S + jc[0]];
        };
        if (n_steps > 0) {
#pragma unroll
            for (int u = 0; u < NSET; ++u) fetch(u, p[u], pe[u]);
        }
        auto step = [&](int o, double (&col)[KCAP], double &pe_o) {
            // lanes at and above S hold y = 0: the columns past S - 1 (copies of column S - 1) add nothing
            double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
#pragma unroll
            for (int k = 0; k < KCAP; k += 4) {
                a0 = fma(ll_bcast(y[0], k), col[k], a0);
                if (k + 1 < KCAP) a1 = fma(ll_bcast(y[0], k + 1), col[k + 1], a1);
                if (k + 2 < KCAP) a2 = fma(ll_bcast(y[0], k + 2), col[k + 2], a2);
                if (k + 3 < KCAP) a3 = fma(ll_bcast(y[0], k + 3), col[k + 3], a3);
            }
            const double dot = (a0 + a1) + (a2 + a3);
            const double x = (dot == 0.0 ? 0.0 : dot * inv_z) + TINY;       // no path in: tiny, whatever 1 / Z is
            const double pe_now = pe_o;
            fetch(o + NSET, col, pe_o);
            y[0] = act[0] ? x * pe_now : 0.0;
            z = wave_sum_dpp(y[0]);
            keep(o + 1, z);
            inv_z = fast_recip_pos(z);
        };
        for (int o = 0; o < n_steps; o += NSET) {
#pragma unroll
            for (int u = 0; u < NSET; ++u)
                if (o + u < n_steps) step(o + u, p[u], pe[u]);
        }
    } else {
        for (int o = 0; o < n_steps; ++o) {
            const double *B = PT + (int64_t)o * bs;
            double pe_now[R];
#pragma unroll
            for (int r = 0; r < R; ++r) pe_now[r] = PE[(int64_t)(o + 1) * S + jc[r]];
            double a[4][R];
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int r = 0; r < R; ++r) a[q][r] = 0.0;
#pragma unroll
            for (int rk = 0; rk < R; ++rk) {
                const int lim = min(64, S - rk * 64);      // source states rk * 64 .. + lim of this register
                for (int l0 = 0; l0 < lim; l0 += 4) {
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const int l = min(l0 + q, lim - 1);
                        const double yk = l0 + q < lim ? ll_bcast(y[rk], l) : 0.0;
                        const double *row = B + (int64_t)(rk * 64 + l) * S;
#pragma unroll
                        for (int r = 0; r < R; ++r) a[q][r] = fma(yk, row[jc[r]], a[q][r]);
                    }
                }
            }
            z_own = 0.0;
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const double dot = (a[0][r] + a[1][r]) + (a[2][r] + a[3][r]);
                const double x = (dot == 0.0 ? 0.0 : dot * inv_z) + TINY;
                y[r] = act[r] ? x * pe_now[r] : 0.0;
                z_own += y[r];
            }
            z = wave_sum_dpp(z_own);
            keep(o + 1, z);
            inv_z = fast_recip_pos(z);
        }
    }
    if (n_genes & 63) flush(n_genes & 63);
    if (lane == 0) out[pair] = bad ? -INFINITY : ll;
}
