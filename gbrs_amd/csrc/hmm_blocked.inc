// Blocked scan for the 36-state recursions of ONE sample (or a few).  Included by hmm.hip inside namespace gbrs.
//
// A chromosome's three recursions (alpha, free-running backward, Viterbi delta; gbrs/gbrs_utils.py:498-579) are chains of
// up to ~3,000 dependent steps of ~0.4 us: one sample is 60 wavefronts on a 1,024-SIMD chip for 1.4 ms.  The recursions
// are products of per-gene operators - sum-product for alpha / backward (x -> pe .* (P x), scale free), max-plus for
// delta (d -> e + max(T + d)) - so a chromosome is cut into B blocks of genes and
//   1. every block's transfer operator (a 36 x 36 matrix: the block's recursion applied to the 36 unit vectors) is
//      computed in parallel: sum-product on v_mfma_f64_16x16x4 with the matrix's columns where alpha_mfma_kernel has
//      its samples (16 columns per wavefront, the emission row shared by all), max-plus with the columns where
//      delta_lanes_kernel has its samples; a column is rescaled by a power of two per step (exact) and the exponents
//      are kept, so the columns stay comparable;
//   2. one wavefront per chromosome applies the block operators to the chromosome's start vector one after the other
//      (B - 1 small matrix-vector products) and leaves every block's incoming boundary vector;
//   3. the chain kernels of hmm.hip run inside ALL blocks at once from those vectors (ChromDesc::inject): same
//      arithmetic, same stored quantities (x, 1/Z, bt, its rescales, delta) as the unblocked run, chains B times shorter.
// The boundary vectors differ from the sequential recursion's by the rounding of a different association (~1e-15
// relative): the log-domain outputs keep their 1e-9, the Viterbi calls are decided by margins of 1e-2 and above
// (tests/test_hmm_gpu.py measures them per chromosome).  `tiny` (the reference adds nextafter(0, 1) inside every
// forward step) is added by the chains as before; a boundary vector carries exact zeros where the sequential chain
// would carry a denormal, which matters only for states of probability below 1e-320.

constexpr int BS_S = 36;
#ifndef HMM_COMBINE_SETS
#define HMM_COMBINE_SETS 2        // operators in flight in combine_sumprod_kernel (measured 2 / 3 / 4: 0.658 / 0.656 / 0.663 ms per pass)
#endif
#ifndef HMM_BS_NSET
#define HMM_BS_NSET 2
#endif

__device__ __forceinline__ int pow2_exponent(double z) {          // e with 2^e <= z < 2^(e+1); 0 for z = 0
    const int hi = __double2hiint(z);
    return z > 0.0 ? ((hi >> 20) & 0x7ff) - 1023 : 0;
}
__device__ __forceinline__ double pow2(int e) {                    // 2^e, -1022 <= e <= 1023
    return __hiloint2double((e + 1023) << 20, 0);
}
// maximum over all 64 lanes, in every lane (DPP inside the rows, the four row results through v_readlane)
__device__ __forceinline__ int wave_max_dpp(int v) {
    v = max(v, __builtin_amdgcn_update_dpp(v, v, DPP_QUAD_XOR1, 0xf, 0xf, false));
    v = max(v, __builtin_amdgcn_update_dpp(v, v, DPP_QUAD_XOR2, 0xf, 0xf, false));
    v = max(v, __builtin_amdgcn_update_dpp(v, v, DPP_ROW_HALF_MIRROR, 0xf, 0xf, false));
    v = max(v, __builtin_amdgcn_update_dpp(v, v, DPP_ROW_MIRROR, 0xf, 0xf, false));
    return max(max(__builtin_amdgcn_readlane(v, 0), __builtin_amdgcn_readlane(v, 16)),
               max(__builtin_amdgcn_readlane(v, 32), __builtin_amdgcn_readlane(v, 48)));
}

// Transfer operator of a block, sum-product.  DIR 0 (alpha): v <- pe_i .* (P_{i-1} v) for i = max(lo, 1) .. hi-1;
// DIR 1 (backward): v <- pe_i .* (P_i^T v) for i = min(hi-1, n-2) .. lo, downwards.  One wavefront per (block, sample)
// carries all 36 columns as three groups of 16 (the last twelve slots shadow column 35): the step's 27 MFMA operands
// are loaded once and used for the three groups in turn - as three wavefronts per block the operand stream
// (14 KB per step and wavefront, 2.2 GB per launch) was what bounded the kernel, not the 81 MFMAs.  The operand layout,
// lane roles and the ones-rows that deliver the vector's sum are alpha_mfma_kernel's.
// out[(sample * n_blocks + block)][column][state], exps[...][column]: column = stored * 2^exp.
template <int DIR>
__global__ void __launch_bounds__(64, HMM_BLK_WAVES)
blockmat_mfma_kernel(int64_t genes_per_sample, int n_slots, const BlockRange *__restrict__ ranges, const double *__restrict__ amat,
                     const double *__restrict__ peprob, double *__restrict__ out, int32_t *__restrict__ exps) {
    constexpr int S = BS_S, NSET = HMM_BS_NSET, NG = 3;
    const BlockRange br = ranges[blockIdx.x];
    if (br.direct || (DIR == 0 ? br.hi >= br.n : br.lo <= 0)) return;   // nobody consumes this block's operator
    const int lane = threadIdx.x, g = lane >> 4;
    const int64_t g0 = (int64_t)blockIdx.y * genes_per_sample + br.gene_off;
    const double *BLK = amat + br.trans_off * (int64_t)MF_BLK;
    const double *pe_row = peprob + g0 * S + 9 * g;
    // steps: gene index i_k and transition block t_k of step k = 0 .. n_steps-1
    const int i_first = DIR == 0 ? max(br.lo, 1) : min(br.hi - 1, br.n - 2);
    const int n_steps = DIR == 0 ? br.hi - i_first : i_first - br.lo + 1;
    const int last_k = max(n_steps - 1, 0);
    auto gene_of = [&](int k) { return DIR == 0 ? i_first + k : i_first - k; };
    auto block_of = [&](int k) { return DIR == 0 ? i_first + k - 1 : i_first - k; };
    double y[NG][MF_Q];
    int esum[NG];
#pragma unroll
    for (int cg = 0; cg < NG; ++cg) {
        const int col = min(cg * 16 + (lane & 15), S - 1);
#pragma unroll
        for (int q = 0; q < MF_Q; ++q) y[cg][q] = (9 * g + q == col) ? 1.0 : 0.0;
        esum[cg] = 0;
    }
    double a[NSET][2 * MF_PAIRS], pe[NSET][MF_Q];
#pragma unroll
    for (int u = 0; u < NSET; ++u) {
        const int k = min(u, last_k);
        if (n_steps > 0) {
            mfma_load_block(BLK + (int64_t)HMM_BLK(block_of(k)) * MF_BLK, lane, a[u]);
            mfma_load_row(pe_row + (int64_t)gene_of(k) * S, pe[u]);
        }
    }
    auto step = [&](int k, const double (&ac)[2 * MF_PAIRS], const double (&pc)[MF_Q], double (&an)[2 * MF_PAIRS], double (&pn)[MF_Q]) {
        double pe_now[MF_Q];
#pragma unroll
        for (int q = 0; q < MF_Q; ++q) pe_now[q] = pc[q];
#pragma unroll
        for (int cg = 0; cg < NG; ++cg) {
            mfma_d4 d0, d1, d2;
            mfma_matvec(ac, y[cg], d0, d1, d2);
            if (cg == NG - 1) {                                  // the set is free once its last product has been issued
                const int kf = min(k + NSET - 1, last_k);
                mfma_load_block(BLK + (int64_t)HMM_BLK(block_of(kf)) * MF_BLK, lane, an);
                mfma_load_row(pe_row + (int64_t)gene_of(kf) * S, pn);
            }
            const int e = pow2_exponent(d2[1]);                 // of the sum of the vector that went in
            const double sc = pow2(-e);
            esum[cg] += e;
#pragma unroll
            for (int q = 0; q < MF_Q; ++q) y[cg][q] = (mfma_own(d0, d1, d2, q) * sc) * pe_now[q];
        }
    };
    int k = 0;
    for (; k + NSET <= n_steps; k += NSET) {
#pragma unroll
        for (int u = 0; u < NSET; ++u) step(k + u, a[u], pe[u], a[(u + NSET - 1) % NSET], pe[(u + NSET - 1) % NSET]);
    }
#pragma unroll
    for (int u = 0; u < NSET - 1; ++u)
        if (k + u < n_steps) step(k + u, a[u], pe[u], a[(u + NSET - 1) % NSET], pe[(u + NSET - 1) % NSET]);
#pragma unroll
    for (int cg = 0; cg < NG; ++cg) {
        const int slot = cg * 16 + (lane & 15);
        if (slot < S) {
            const int64_t at = ((int64_t)blockIdx.y * n_slots + blockIdx.x) * S + slot;
            mfma_store_row(out + at * S + 9 * g, y[cg]);
            if (g == 0) exps[at] = esum[cg];
        }
    }
}

// Phase 2, sum-product: the chromosome's start vector through the block operators, one after the other; the vector that
// enters block v (forward: y of gene lo-1, any scale; backward: pe .* bt of gene hi) goes to inject[sample][v][state].
// One wavefront per (chromosome, sample); lane j owns state j.  first_block[c] .. first_block[c+1]: the chromosome's blocks.
template <int DIR>
__global__ void __launch_bounds__(64)
combine_sumprod_kernel(int64_t genes_per_sample, int n_blocks, const BlockRange *__restrict__ ranges,
                       const int32_t *__restrict__ first_block, const double *__restrict__ mats,
                       const int32_t *__restrict__ exps, const double *__restrict__ init_vec,
                       const double *__restrict__ eprob, const double *__restrict__ peprob,
                       const double *__restrict__ stored /* forward: x of every gene (xsum); backward: bt (bhat) */,
                       double *__restrict__ inject) {
    constexpr int S = BS_S;
    __shared__ double w[64];
#if defined(HMM_COMBINE_PRIO)                    // experiment: the 20 combine wavefronts (the pass's critical path) ahead of the chains
    __builtin_amdgcn_s_setprio(HMM_COMBINE_PRIO);
#endif
    const int c = blockIdx.x, sample = blockIdx.y, j = threadIdx.x;
    const int v0 = first_block[c], v1 = first_block[c + 1];
    if (v1 - v0 < 2) return;
    const bool act = j < S;
    const int jr = act ? j : S - 1;
    const BlockRange b0 = ranges[v0];
    const int64_t g0 = (int64_t)sample * genes_per_sample + b0.gene_off;
    const int64_t base = (int64_t)sample * n_blocks;
    // A directly chained first (forward) / last (backward) block has no operator: the vector that enters its neighbour is
    // what its chain stored - forward: y = x .* pe of its last gene, backward: pe .* bt of its first gene (any scale).
    const BlockRange bd = ranges[DIR == 0 ? v0 : v1 - 1];
    const bool direct = bd.direct != 0;
    double vec;
    if (direct) {
        const int64_t gd = (g0 + (DIR == 0 ? bd.hi - 1 : bd.lo)) * S + jr;
        vec = stored[gd] * peprob[gd];
        if (act) inject[(base + (DIR == 0 ? v0 + 1 : v1 - 2)) * S + j] = vec;
    } else {
        vec = DIR == 0 ? exp(init_vec[jr] + eprob[g0 * S + jr]) : peprob[(g0 + b0.n - 1) * S + jr];
    }
    if (!act) vec = 0.0;
    // forward: operators of blocks v0 .. v1-2 feed blocks v0+1 .. v1-1; backward: operators of v1-1 .. v0+1 feed v1-2 .. v0
    const int n_ops = v1 - v0 - 1;
    auto op_block = [&](int t) { return DIR == 0 ? v0 + t : v1 - 1 - t; };
    auto fed_block = [&](int t) { return DIR == 0 ? v0 + t + 1 : v1 - 2 - t; };
    // COMBINE_SETS register sets used in turn: the operators (and exponents) of the next steps are on their way while the
    // current one is applied - beside the chain kernels an operator's 10 KB take longer to arrive than a step takes
    constexpr int NCS = HMM_COMBINE_SETS;
    double gR[NCS][S];
    int exR[NCS];
#pragma unroll
    for (int u = 0; u < NCS; ++u) exR[u] = 0;
    auto load_op = [&](int t, double (&dst)[S], int &ex) {
        const double *m = mats + (base + op_block(t)) * (int64_t)(S * S) + jr;
#pragma unroll
        for (int cc = 0; cc < S; ++cc) dst[cc] = m[cc * S];
        ex = exps[(base + op_block(t)) * S + jr];
    };
    auto apply = [&](int t, const double (&gcol)[S], int ex) {
        // column cc of the operator is stored * 2^exp: fold the exponents into the vector, relative to the largest term
        const int tj = (act && vec > 0.0) ? ex + pow2_exponent(vec) : -(1 << 28);
        const int tmax = wave_max_dpp(tj);
        const int sh = ex - tmax;
        double wj = 0.0;
        if (act && vec > 0.0 && sh > -1000) wj = vec * pow2(max(sh, -1000));
        // one wavefront: its LDS instructions execute in order, no barrier (a __syncthreads would also wait for the
        // next operator's loads, which are meant to stay in flight across this step)
        wave_lds_fence();
        w[j] = wj;
        wave_lds_fence();
        double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
#pragma unroll
        for (int cc = 0; cc < S; cc += 4) {
            a0 = fma(gcol[cc], w[cc], a0);
            a1 = fma(gcol[cc + 1], w[cc + 1], a1);
            a2 = fma(gcol[cc + 2], w[cc + 2], a2);
            a3 = fma(gcol[cc + 3], w[cc + 3], a3);
        }
        const double r = act ? (a0 + a1) + (a2 + a3) : 0.0;
        const double tot = wave_sum_dpp(r);
        vec = tot > 0.0 ? r * fast_recip_pos(tot) : r;             // any positive scale would do
        if (act) inject[(base + fed_block(t)) * S + j] = vec;
    };
    const int t0 = direct ? 1 : 0;                                  // (the direct block's neighbour has its vector already)
#pragma unroll
    for (int u = 0; u < NCS; ++u)
        if (t0 + u < n_ops) load_op(t0 + u, gR[u], exR[u]);
    for (int t = t0; t < n_ops; t += NCS) {
#pragma unroll
        for (int u = 0; u < NCS; ++u) {
            if (t + u < n_ops) {                                    // wave-uniform
                apply(t + u, gR[u], exR[u]);
                if (t + u + NCS < n_ops) load_op(t + u + NCS, gR[u], exR[u]);
            }
        }
    }
}

// Transfer operator of a block, max-plus (Viterbi): d <- e_i + max_k(T_{i-1}[.][k] + d[k]) for i = max(lo, 1) .. hi-1,
// started from the 36 unit vectors of the max-plus algebra (0 at the column's own state, -inf elsewhere).
// out[(sample * n_blocks + block)][column][state].
//
// One workgroup of seven wavefronts per block.  A 16-lane row is (target group tg, column group cg): its lanes are 16
// columns of the operator and it owns the FOUR target states 4 tg .. 4 tg + 3 (9 groups x 3 column groups = 27 rows).
// A lane reads its column's 36 previous values from LDS once per step and uses them for its four targets; the
// 4 x 36 transition entries of the row's targets are 144 consecutive doubles of the block, nine registers across
// the row's 16 lanes, and enter the additions through the DPP row broadcast of v_fmac_f64 as in delta_lanes_kernel
// (entry * 1.0 + previous: one rounding of the exact sum, the value the addition gives).  Against delta_lanes_kernel's
// one target per lane this reads every previous value from LDS 9 times instead of 36 times per step - there the LDS
// pipe, not the 72 double-precision instructions per lane, set the step time.
constexpr int MP_ROWS = 27, MP_WAVES = 7, MP_COLS = 48, MP_TREGS = 9;

// v_max_f64 as written: fmax() on a value that comes out of inline asm is preceded by a canonicalising max(x, x)
// (the compiler cannot see that v_fmac_f64 already quieted it) - one extra instruction per pair
__device__ __forceinline__ double max_f64(double a, double b) {
    double r;
    asm("v_max_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}

// targets JT = 0..3 of the row, sources K = 0..35: entry JT * 36 + K sits in register (JT * 36 + K) / 16, lane % 16
template <int JT, int K>
__device__ __forceinline__ void mp_from(const double (&t)[MP_TREGS], const double (&dp)[MF_S], double one, double (&m)[4][2]) {
    constexpr int E = JT * MF_S + K;
    const double a = add_row_bcast<E % 16>(dp[K], t[E / 16], one);
    if constexpr (K < 2) m[JT][K & 1] = a; else m[JT][K & 1] = max_f64(m[JT][K & 1], a);
    if constexpr (JT < 3) mp_from<JT + 1, K>(t, dp, one, m);          // the four targets side by side: independent instructions
    else if constexpr (K + 1 < MF_S) mp_from<0, K + 1>(t, dp, one, m);
}

__global__ void __launch_bounds__(64 * MP_WAVES)
blockmat_maxplus_kernel(int64_t genes_per_sample, int n_slots, const BlockRange *__restrict__ ranges, const double *__restrict__ tprob,
                        const double *__restrict__ eprob, double *__restrict__ out) {
    constexpr int S = MF_S, BLK = S * S, NT = 64 * MP_WAVES, TPT = (BLK + NT - 1) / NT;
    __shared__ __attribute__((aligned(16))) double dbuf[2][MP_COLS][DL_STRIDE];
    // the step's transition block, staged once per workgroup (every row group of the 27 needs 144 of its entries, the
    // three column groups the same ones: fetched per row from global memory the launch moved 1.6 GB through L2 and
    // that, not its arithmetic, was its time)
    __shared__ __attribute__((aligned(16))) double tbuf[2][BLK];
    const BlockRange br = ranges[blockIdx.x];
    if (br.direct || br.hi >= br.n) return;
    const int tid = threadIdx.x, c = tid & 15;
    const int row = min(tid >> 4, MP_ROWS - 1);                    // the 28th row shadows the 27th (same values, same stores)
    const int tg = row % 9, cg = row / 9;
    const int slot = cg * 16 + c, col = min(slot, S - 1);          // column slots past 35 shadow column 35
    const int64_t g0 = (int64_t)blockIdx.y * genes_per_sample + br.gene_off;
    const int i_first = max(br.lo, 1), n_steps = br.hi - i_first;
    const int last_k = max(n_steps - 1, 0);
    const double *e_at = eprob + g0 * S + 4 * tg;                   // + i * S: my four targets of gene i
    const double *TB = tprob + br.trans_off * (int64_t)BLK;
    double one = 1.0;
    asm volatile("" : "+v"(one));
    // global -> registers two steps ahead, registers -> LDS one step ahead
    double t_in[TPT];
    auto fetch_block = [&](int k) {
        const double *src = TB + (int64_t)HMM_BLK(i_first + min(k, last_k) - 1) * BLK;
#pragma unroll
        for (int u = 0; u < TPT; ++u) t_in[u] = src[min(tid + u * NT, BLK - 1)];
    };
    auto stage_block = [&](int k) {
#pragma unroll
        for (int u = 0; u < TPT; ++u)
            if (tid + u * NT < BLK) tbuf[k & 1][tid + u * NT] = t_in[u];
    };
    double2 e_now[2], e_next[2];
    auto fetch_e = [&](int k, double2 (&e)[2]) {
        const double2 *ep = reinterpret_cast<const double2 *>(e_at + (int64_t)(i_first + min(k, last_k)) * S);
        e[0] = ep[0];
        e[1] = ep[1];
    };
    {
        double *d0 = &dbuf[0][slot][4 * tg];
#pragma unroll
        for (int jt = 0; jt < 4; ++jt) d0[jt] = (4 * tg + jt == col) ? 0.0 : -INFINITY;
    }
    if (n_steps > 0) {
        fetch_block(0);
        stage_block(0);
        fetch_block(1);
        fetch_e(0, e_now);
    }
    __syncthreads();
    int cur = 0;
    for (int k = 0; k < n_steps; ++k) {
        double tr[MP_TREGS];
        const double *tsrc = &tbuf[k & 1][4 * tg * S + c];
#pragma unroll
        for (int m = 0; m < MP_TREGS; ++m) tr[m] = tsrc[16 * m];
        double dp[S];
        const mf_pair *src = reinterpret_cast<const mf_pair *>(&dbuf[cur][slot][0]);
#pragma unroll
        for (int k2 = 0; k2 < S / 2; ++k2) {
            const mf_pair pr = src[k2];
            dp[2 * k2] = pr.x;
            dp[2 * k2 + 1] = pr.y;
        }
        fetch_e(k + 1, e_next);
        stage_block(k + 1);                                         // block k+1: in registers since the previous step
        fetch_block(k + 2);
        double m[4][2];
        mp_from<0, 0>(tr, dp, one, m);
        mf_pair *dst = reinterpret_cast<mf_pair *>(&dbuf[cur ^ 1][slot][4 * tg]);
        dst[0] = mf_pair{max_f64(m[0][0], m[0][1]) + e_now[0].x, max_f64(m[1][0], m[1][1]) + e_now[0].y};
        dst[1] = mf_pair{max_f64(m[2][0], m[2][1]) + e_now[1].x, max_f64(m[3][0], m[3][1]) + e_now[1].y};
        e_now[0] = e_next[0];
        e_now[1] = e_next[1];
        cur ^= 1;
        __syncthreads();
    }
    if (slot < S) {
        double *o = out + (((int64_t)blockIdx.y * n_slots + blockIdx.x) * S + col) * S + 4 * tg;
#pragma unroll
        for (int jt = 0; jt < 4; ++jt) o[jt] = dbuf[cur][slot][4 * tg + jt];
    }
}

// Phase 2, max-plus: delta of the gene before every block's first one.
__global__ void __launch_bounds__(64)
combine_maxplus_kernel(int64_t genes_per_sample, int n_blocks, const BlockRange *__restrict__ ranges,
                       const int32_t *__restrict__ first_block, const double *__restrict__ mats,
                       const double *__restrict__ init_vec, const double *__restrict__ eprob,
                       const double *__restrict__ delta /* what a directly chained first block stored */, double *__restrict__ inject) {
    constexpr int S = BS_S;
    __shared__ double w[64];
    const int c = blockIdx.x, sample = blockIdx.y, j = threadIdx.x;
    const int v0 = first_block[c], v1 = first_block[c + 1];
    if (v1 - v0 < 2) return;
    const bool act = j < S;
    const int jr = act ? j : S - 1;
    const BlockRange b0 = ranges[v0];
    const int64_t g0 = (int64_t)sample * genes_per_sample + b0.gene_off;
    const int64_t base = (int64_t)sample * n_blocks;
    const bool direct = b0.direct != 0;
    double vec;
    if (direct) {                                    // delta of the first block's last gene, exactly as the chain left it
        vec = delta[(g0 + b0.hi - 1) * S + jr];
        if (act) inject[(base + v0 + 1) * S + j] = vec;
    } else {
        vec = init_vec[jr] + eprob[g0 * S + jr];
    }
    double gA[S], gB[S];
    auto load_op = [&](int t, double (&dst)[S]) {
        const double *m = mats + (base + v0 + t) * (int64_t)(S * S) + jr;
#pragma unroll
        for (int cc = 0; cc < S; ++cc) dst[cc] = m[cc * S];
    };
    const int n_ops = v1 - v0 - 1;
    auto apply = [&](int t, const double (&gcol)[S]) {
        wave_lds_fence();
        w[j] = vec;
        wave_lds_fence();
        double m0 = gcol[0] + w[0], m1 = gcol[1] + w[1], m2 = gcol[2] + w[2], m3 = gcol[3] + w[3];
#pragma unroll
        for (int cc = 4; cc < S; cc += 4) {
            m0 = fmax(m0, gcol[cc] + w[cc]);
            m1 = fmax(m1, gcol[cc + 1] + w[cc + 1]);
            m2 = fmax(m2, gcol[cc + 2] + w[cc + 2]);
            m3 = fmax(m3, gcol[cc + 3] + w[cc + 3]);
        }
        vec = fmax(fmax(m0, m1), fmax(m2, m3));
        if (act) inject[(base + v0 + t + 1) * S + j] = vec;
    };
    const int t0 = direct ? 1 : 0;
    if (t0 < n_ops) load_op(t0, gA);
    for (int t = t0; t < n_ops; t += 2) {
        if (t + 1 < n_ops) load_op(t + 1, gB);
        apply(t, gA);
        if (t + 1 < n_ops) {
            if (t + 2 < n_ops) load_op(t + 2, gA);
            apply(t + 1, gB);
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------------
// Viterbi values without block operators (round 4): rank convergence of the max-plus recursion.
//
// d -> e + max(T + d) commutes with adding a constant to d, and after a few genes with informative emissions the best
// paths from all 36 start states run through one state: from there on the recursion's value no longer depends on the
// vector it was started from, except for that constant.  So instead of 36 unit vectors per block (blockmat_maxplus_kernel:
// 36 x the work of the chain, the largest cost of the one-sample pass) every block is chained ONCE from a guess:
//   1. delta_guess_kernel: block v's start vector := the emission row of the gene before it (any vector would do);
//   2. the chain kernel (forward_wave_kernel, role 1) inside all blocks at once, as in the operator scheme;
//   3. delta_fixup_kernel, all blocks at once: the chain again from what the PREVIOUS block stored for its last gene - which
//      is the true vector minus that block's constant -, gene by gene, until it differs from what step 2 stored for this
//      block by one constant over all states (spread <= tol): the genes before that point are overwritten, the constant is
//      recorded, the rest of the block keeps its stored values.  Every stored 36-vector is then the true one minus ONE
//      constant, which is all the backpointers (argmax_k(delta[k] + T[j][k])), the backtrace and argmax(delta[:, n-1]) need;
//   4. delta_apply_kernel (after the backpointers): adds the running sums of the constants, so that `delta` holds the
//      values of the sequential recursion (rounding of a different association, ~1e-15 relative, as with the operators).
//   5. the backtrace (backtrace_write_kernel, TieCheck) takes best minus second best of every decision of the path it writes:
//      a decision closer than twice the fix-up's acceptance spread - an exact tie, a near-tie: the stored vectors cannot
//      decide it as the sequential chain does - raises the chromosome's flag, and the host, which reads the flags when the
//      pass is done, sends the chromosome through the unblocked chain and the backtrace once more.
// A block whose fix-up reaches its last gene without meeting the stored values (a stretch of genes without information as
// long as a block) raises the chromosome's flag, and the unblocked chain kernel, launched behind the fix-up and idle
// otherwise (`only_if`), recomputes that chromosome.  Measured on the synthetic samples: SURVEY's tables converge within
// 2 genes (median; 7 at most), DO-like tables (recombination 1e-15 .. 1e-2, structural zeros) with 10 % of the haplotypes
// expressed within 9 (34 at most); blocks are ~40 genes.
// ------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(64)
delta_guess_kernel(int64_t genes_per_sample, int n_slots, int n_chrom, const BlockRange *__restrict__ ranges,
                   const double *__restrict__ eprob, double *__restrict__ inject, double *__restrict__ c_rel,
                   int32_t *__restrict__ gstar, int32_t *__restrict__ fail, int32_t *__restrict__ tie) {
    constexpr int S = BS_S;
    const BlockRange r = ranges[blockIdx.x];
    const int j = threadIdx.x, sample = blockIdx.y;
    const int64_t slot = (int64_t)sample * n_slots + blockIdx.x;
    if (j == 0) {
        c_rel[slot] = 0.0;
        gstar[slot] = r.lo;
        if (r.lo == 0) fail[sample * n_chrom + r.chrom] = tie[sample * n_chrom + r.chrom] = 0;
    }
    if (r.lo == 0 || j >= S) return;
    inject[slot * S + j] = eprob[((int64_t)sample * genes_per_sample + r.gene_off + r.lo - 1) * S + j];
}

template <int SS>
__global__ void __launch_bounds__(64, HMM_BLK_WAVES)
delta_fixup_kernel(int64_t genes_per_sample, int n_slots, int n_chrom, const BlockRange *__restrict__ ranges,
                   const double *__restrict__ tprob_q, const double *__restrict__ eprob, double *__restrict__ delta,
                   double *__restrict__ c_rel, int32_t *__restrict__ gstar, int32_t *__restrict__ fail, double tol_abs,
                   double tol_rel, uint16_t *__restrict__ bp, int64_t bp_per_sample) {
    __shared__ __attribute__((aligned(16))) double buf[2][SS];
    __shared__ __attribute__((aligned(16))) double sdiff[SS];
    const BlockRange r = ranges[blockIdx.x];
    if (r.lo == 0) return;                           // a chromosome's first block starts from the true vector
    const int j = threadIdx.x, sample = blockIdx.y;
    const bool act = j < SS;
    const int jr = act ? j : SS - 1;
    const int64_t slot = (int64_t)sample * n_slots + blockIdx.x;
    const int64_t g_base = (int64_t)sample * genes_per_sample + r.gene_off;
    const double *TB = tprob_q + (r.trans_off + r.lo - 1) * (int64_t)SS * SS;     // step o (gene lo + o) reads block o
    const int n_steps = r.hi - r.lo;
    if (act) buf[0][j] = delta[(g_base + r.lo - 1) * SS + j];
    wave_lds_fence();
    int cur = 0;
    // One register set, loads issued at the top of the step: a fix-up is a handful of steps (the load's latency shows, ~1 us
    // each), and ~1,000 of these wavefronts should fit beside the other kernels of the pass.
    for (int o = 0; o < n_steps; ++o) {
        double t_row[SS];
        load_lane<SS>(TB + (int64_t)o * SS * SS, jr, t_row);
        const double e = eprob[(g_base + r.lo + o) * SS + jr];
        const double dp = delta[(g_base + r.lo + o) * SS + jr];
        const double2 *pv = reinterpret_cast<const double2 *>(buf[cur]);
        double m0, m1, m2, m3;
        int k0 = 0, k1 = 1, k2 = 2, k3 = 3;
        {
            const double2 a = pv[0], b = pv[1];
            m0 = a.x + t_row[0]; m1 = a.y + t_row[1]; m2 = b.x + t_row[2]; m3 = b.y + t_row[3];
        }
#pragma unroll
        for (int m = 2; m < SS / 2; ++m) {
            const double2 v = pv[m];
            const double a = v.x + t_row[2 * m], c = v.y + t_row[2 * m + 1];
            if (m & 1) { k2 = a > m2 ? 2 * m : k2; k3 = c > m3 ? 2 * m + 1 : k3; m2 = fmax(m2, a); m3 = fmax(m3, c); }
            else { k0 = a > m0 ? 2 * m : k0; k1 = c > m1 ? 2 * m + 1 : k1; m0 = fmax(m0, a); m1 = fmax(m1, c); }
        }
        // this step's backpointer row (of gene lo - 1 + o) from the true vector: what the chain wrote for it came from the guess
        // (o = 0) or from values the fix-up is replacing
        if (act) bp[((int64_t)sample * bp_per_sample + r.bp_off + r.lo - 1 + o) * SS + j] = (uint16_t)first_max4(m0, k0, m1, k1, m2, k2, m3, k3);
        const double d = fmax(fmax(m0, m1), fmax(m2, m3)) + e;
        if (act) {
            sdiff[j] = d - dp;                       // -inf - -inf = NaN: skipped by fmax / fmin below
            buf[cur ^ 1][j] = d;
        }
        cur ^= 1;
        wave_lds_fence();
        const double2 *sv = reinterpret_cast<const double2 *>(sdiff);
        const double2 *tv = reinterpret_cast<const double2 *>(buf[cur]);
        double mx = -INFINITY, mn = INFINITY, mag = 0.0;
#pragma unroll
        for (int m = 0; m < SS / 2; ++m) {
            const double2 v = sv[m], w = tv[m];
            mx = fmax(mx, fmax(v.x, v.y));
            mn = fmin(mn, fmin(v.x, v.y));
            const double ax = fabs(w.x), ay = fabs(w.y);
            mag = fmax(mag, fmax(ax < INFINITY ? ax : 0.0, ay < INFINITY ? ay : 0.0));
        }
        const bool none = !(mx >= mn);               // every state -inf on both sides
        if (none || mx - mn <= tol_abs + tol_rel * mag) {     // met the stored values: they stand from this gene on
            if (j == 0) {
                c_rel[slot] = none ? 0.0 : 0.5 * (mx + mn);
                gstar[slot] = r.lo + o;
            }
            return;
        }
        if (o == n_steps - 1) {                      // the block's last gene reached without meeting them
            if (j == 0) fail[sample * n_chrom + r.chrom] = 1;
            return;
        }
        if (act) delta[(g_base + r.lo + o) * SS + j] = d;
        wave_lds_fence();                            // sdiff is rewritten by the next step
    }
}

// delta as the sequential recursion has it: every block's stored vectors plus the constants of the blocks before it (and its
// own from the gene on where its fix-up met the stored values).  The running sums are taken serially, in block order, by
// every wavefront itself, so that neighbouring blocks use bit-identical constants.
__global__ void __launch_bounds__(64)
delta_apply_kernel(int64_t genes_per_sample, int n_slots, int n_chrom, const BlockRange *__restrict__ ranges,
                   const int32_t *__restrict__ first_block, const double *__restrict__ c_rel,
                   const int32_t *__restrict__ gstar, const int32_t *__restrict__ fail, const int32_t *__restrict__ tie,
                   double *__restrict__ delta) {
    constexpr int S = BS_S;
    const BlockRange r = ranges[blockIdx.x];
    const int sample = blockIdx.y;
    if (r.lo == 0 || fail[sample * n_chrom + r.chrom] || tie[sample * n_chrom + r.chrom]) return;   // recomputed: the chain's own values
    const int64_t base = (int64_t)sample * n_slots;
    double c_prev = 0.0;
    for (int u = first_block[r.chrom]; u < (int)blockIdx.x; ++u) c_prev += c_rel[base + u];
    const double c_own = c_prev + c_rel[base + blockIdx.x];
    const int split = (gstar[base + blockIdx.x] - r.lo) * S;
    double *d = delta + ((int64_t)sample * genes_per_sample + r.gene_off + r.lo) * S;
    const int total = (r.hi - r.lo) * S;
    for (int x = threadIdx.x; x < total; x += 64) d[x] += x < split ? c_prev : c_own;
}

// The free-running backward chains of the blocks rescale on their own, and a block starts from a boundary vector of
// arbitrary scale: relative to the values the NEXT block stored, the first step of block v carries the extra factor
// rho_v = sum(pe_hi .* bt_hi as stored) / sum(injected vector).  Folding it into that step's recorded rescale makes the
// blocks one free-running chain again, which is what beta_corr_kernel's suffix sums assume (beta on demand only).
__global__ void __launch_bounds__(64)
blocked_bscale_fix_kernel(int64_t genes_per_sample, int n_blocks, const BlockRange *__restrict__ ranges,
                          const double *__restrict__ peprob, const double *__restrict__ bhat,
                          const double *__restrict__ inject, double *__restrict__ bscale) {
    constexpr int S = BS_S;
    const BlockRange br = ranges[blockIdx.x];
    if (br.hi >= br.n) return;
    const int j = threadIdx.x, sample = blockIdx.y;
    const int64_t g0 = (int64_t)sample * genes_per_sample + br.gene_off;
    double a = 0.0, b = 0.0;
    if (j < S) {
        a = peprob[(g0 + br.hi) * S + j] * bhat[(g0 + br.hi) * S + j];
        b = inject[((int64_t)sample * n_blocks + blockIdx.x) * S + j];
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        a += __shfl_xor(a, off, 64);
        b += __shfl_xor(b, off, 64);
    }
    if (j == 0 && a > 0.0 && b > 0.0) bscale[g0 + br.hi - 1] *= b / a;
}
