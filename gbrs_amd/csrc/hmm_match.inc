// Match pass of the HMM handle (gbrs_hmm_set_panel / gbrs_hmm_match; DESIGN.md §25): the grid dosages of a launch's samples
// against the dosages of a panel of reference animals on the same grid, per chromosome
//   cross[s][c][j] = sum over the grid points p of c and the founders h of a[s][p][h] * b[j][p][h]
// and the two squared norms.  Included by hmm_passes.hip inside namespace gbrs.
//
// Both operands are row-major with K contiguous: a sample's row is its `grid_dosage` block ([grid point][H], the
// chromosomes in handle order), a panel entry's row has the same layout, so chromosome c is the columns
// [point_off * H, (point_off + n_points) * H) of both and the product is A_c (n x K_c) * B_c^T (K_c x M).

// A workgroup of four wavefronts owns a block of 64 samples x 64 panel entries of one chromosome and walks K_c in chunks
// of MT_KC columns: the two 64 x MT_KC operand blocks go to LDS (rows MT_LD doubles apart), wavefront w multiplies the
// samples 16 w .. 16 w + 15 with all 64 entries, four 16x16 accumulators on v_mfma_f64_16x16x4_f64 (operand maps above
// mfma_blocks_kernel in hmm.hip: A[i = lane & 15][k = lane >> 4], B[k = lane >> 4][n = lane & 15], register r of lane
// (g, n) is D[g + 4 r][n]).  A k step reads one A value and four B values per lane for four MFMAs.
// LDS rows are MT_KC + 2 doubles apart: a ds_read_b64 serves lanes 0-31 and 32-63 in one cycle each, lane (i, g) reads
// double MT_LD * i + g + const, and with MT_LD = 2 (mod 32) the 32 lanes of a half (16 rows x 2 values of g) fall on 32
// different bank pairs.  The stride is even, so the staging stores stay 16-byte aligned.
// Determinism: an (s, c, j) sum is formed by one wavefront, chunk after chunk, k step after k step, and nothing in that
// order looks at n, M or where the sample and the entry sit in their blocks; there is no atomic and K is not split.
// Rows past the last sample and entries past the last panel entry shadow the last one (same loads, their results are
// not stored), as the MFMA sweeps shadow the last sample.  The chunk loop has no predicate; the K tail (K_c mod MT_KC
// columns, the whole of K_c at H = 1 or 3 with one grid point) is one more chunk staged with zero fill after the loop,
// and only that staging is predicated: nothing reads past the chromosome's columns, so nothing reads past a row's end.
constexpr int MT_ROWS = 64, MT_COLS = 64, MT_KC = 32, MT_LD = MT_KC + 2, MT_THREADS = 256;
static_assert(MT_LD % 32 == 2 && MT_KC % 4 == 0, "see the bank argument above");
static_assert(MT_ROWS == 16 * (MT_THREADS / 64) && MT_COLS == 64, "16 samples per wavefront, four column tiles");

// One 64 x MT_KC operand block on its way to LDS, in two halves: match_fetch reads a thread's MT_PER values from memory
// into registers, match_put stores them to LDS.  src: column 0 of the chunk in row 0 of the operand; rows first + r,
// clamped to the last row.  VEC2: ld and the chunk's first column are even, so every pair of columns is one aligned
// 16-byte load, 16 lanes across the 256 contiguous bytes of a row, and one 16-byte LDS store.  TAIL: the columns from
// `valid` on are zeros and are not read.
constexpr int MT_PER = MT_ROWS * MT_KC / MT_THREADS;
template <bool VEC2, bool TAIL>
__device__ __forceinline__ void match_fetch(double (&v)[MT_PER], const double *__restrict__ src, int64_t ld, int first,
                                            int n_rows, int valid) {
    const int t = threadIdx.x;
    if constexpr (VEC2 && !TAIL) {
#pragma unroll
        for (int i = 0; i < MT_PER / 2; ++i) {
            const int idx = t + MT_THREADS * i, r = idx / (MT_KC / 2), k = 2 * (idx % (MT_KC / 2));
            const double2 x = *reinterpret_cast<const double2 *>(src + (int64_t)min(first + r, n_rows - 1) * ld + k);
            v[2 * i] = x.x;
            v[2 * i + 1] = x.y;
        }
    } else {
#pragma unroll
        for (int i = 0; i < MT_PER; ++i) {
            const int idx = t + MT_THREADS * i, r = idx / MT_KC, k = idx % MT_KC;
            const double *row = src + (int64_t)min(first + r, n_rows - 1) * ld;
            if constexpr (TAIL) v[i] = k < valid ? row[k] : 0.0;
            else v[i] = row[k];
        }
    }
}

template <bool VEC2>
__device__ __forceinline__ void match_put(double *dst, const double (&v)[MT_PER]) {
    const int t = threadIdx.x;
    if constexpr (VEC2) {
#pragma unroll
        for (int i = 0; i < MT_PER / 2; ++i) {
            const int idx = t + MT_THREADS * i, r = idx / (MT_KC / 2), k = 2 * (idx % (MT_KC / 2));
            *reinterpret_cast<double2 *>(dst + r * MT_LD + k) = double2{v[2 * i], v[2 * i + 1]};
        }
    } else {
#pragma unroll
        for (int i = 0; i < MT_PER; ++i) {
            const int idx = t + MT_THREADS * i;
            dst[(idx / MT_KC) * MT_LD + idx % MT_KC] = v[i];
        }
    }
}

// blockIdx.x: block of 64 samples (fastest, so the sample blocks that share a panel block run side by side and the panel
// block comes from HBM once for the launch), blockIdx.y: block of 64 panel entries, blockIdx.z: chromosome on the grid.
// cross is [n][n_chrom][M].
// K_c is one chain of dependent MFMAs per accumulator and cannot be split, so what a chunk costs is what the pass costs:
// the loads of chunk m + 1 are issued into registers before the MFMAs of chunk m and stored to LDS after them, so a
// chunk takes the longer of its memory latency and its 32 MFMAs per wavefront, not their sum.  The loop runs over the
// chunks that have a successor and the last full chunk follows it, so the prefetch needs no predicate either.
template <bool VEC2>
__global__ void __launch_bounds__(MT_THREADS)
match_cross_kernel(int n, int M, int n_chrom, int64_t ld, const MatchChrom *__restrict__ chroms, const double *__restrict__ a,
                   const double *__restrict__ b, double *__restrict__ cross) {
    __shared__ __attribute__((aligned(16))) double lds_a[MT_ROWS * MT_LD];
    __shared__ __attribute__((aligned(16))) double lds_b[MT_COLS * MT_LD];
    const MatchChrom c = chroms[blockIdx.z];
    const int row0 = blockIdx.x * MT_ROWS, col0 = blockIdx.y * MT_COLS;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, i = lane & 15, g = lane >> 4;
    mfma_d4 acc[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) acc[t] = mfma_d4{0.0, 0.0, 0.0, 0.0};
    const double *ra = lds_a + (wave * 16 + i) * MT_LD + g, *rb = lds_b + i * MT_LD + g;
    auto multiply = [&]() {
#pragma unroll
        for (int kk = 0; kk < MT_KC; kk += 4) {
            const double av = ra[kk];
#pragma unroll
            for (int t = 0; t < 4; ++t) acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, rb[t * 16 * MT_LD + kk], acc[t], 0, 0, 0);
        }
    };
    const double *pa = a + c.k_off, *pb = b + c.k_off;
    const int64_t chunks = c.k_len / MT_KC;
    double va[MT_PER], vb[MT_PER];
    if (chunks > 0) {
        match_fetch<VEC2, false>(va, pa, ld, row0, n, 0);
        match_fetch<VEC2, false>(vb, pb, ld, col0, M, 0);
        for (int64_t m = 1; m < chunks; ++m) {
            match_put<VEC2>(lds_a, va);
            match_put<VEC2>(lds_b, vb);
            __syncthreads();
            match_fetch<VEC2, false>(va, pa + m * MT_KC, ld, row0, n, 0);
            match_fetch<VEC2, false>(vb, pb + m * MT_KC, ld, col0, M, 0);
            multiply();
            __syncthreads();
        }
        match_put<VEC2>(lds_a, va);
        match_put<VEC2>(lds_b, vb);
        __syncthreads();
        multiply();
        __syncthreads();
    }
    const int tail = (int)(c.k_len - chunks * MT_KC);
    if (tail) {
        match_fetch<false, true>(va, pa + chunks * MT_KC, ld, row0, n, tail);
        match_fetch<false, true>(vb, pb + chunks * MT_KC, ld, col0, M, tail);
        match_put<false>(lds_a, va);
        match_put<false>(lds_b, vb);
        __syncthreads();
        multiply();
    }
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = row0 + wave * 16 + g + 4 * r, col = col0 + t * 16 + i;
            if (row < n && col < M) cross[((int64_t)row * n_chrom + c.chrom) * M + col] = acc[t][r];
        }
}

// Squared norm of every (row, chromosome of the handle): one wavefront each, lanes across the columns, every lane adds its
// squares in column order and the 64 sums meet in a butterfly, so the order depends on the chromosome alone.  A
// chromosome without grid points gives 0.0.  out is [rows][n_chrom].
__global__ void __launch_bounds__(64)
match_norm_kernel(int H, int64_t ld, const GridChrom *__restrict__ chroms, const double *__restrict__ x, double *__restrict__ out) {
    const GridChrom c = chroms[blockIdx.y];
    const double *row = x + (int64_t)blockIdx.x * ld + (int64_t)c.point_off * H;
    const int64_t len = (int64_t)c.n_points * H;
    double acc = 0.0;
#pragma unroll 4
    for (int64_t k = threadIdx.x; k < len; k += 64) {
        const double v = row[k];
        acc += v * v;
    }
    acc = wave_sum_all(acc);
    if (threadIdx.x == 0) out[(int64_t)blockIdx.x * gridDim.y + blockIdx.y] = acc;
}
