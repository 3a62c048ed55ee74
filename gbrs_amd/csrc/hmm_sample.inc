// Diplotype paths drawn from the joint posterior of the last run (gbrs_hmm_sample_paths; DESIGN.md §22): forward-filter /
// backward-sample on the filtered forward values that hmm_make_logs leaves as `alpha` ([sample][gene][S], logs) and the
// handle's log transition tables T[i][to][from] in their uploaded order.  Included by hmm_passes.hip inside namespace gbrs.
//
// Draw d of sample s on chromosome c, genes i = n-1 .. 0:
//   l_k = alpha[i][k]                            at the last gene,
//   l_k = alpha[i][k] + T[i][z_{i+1}][k]         below it;          w_k = exp(l_k),  c_k = w_0 + .. + w_k,  t = u * c_{S-1},
//   z_i = the smallest k with c_k > t;  none by rounding: the largest k with w_k > 0;  c_{S-1} zero or not finite: the
//   first argmax of l_k, and the call's `degenerate` count goes up by one.
//   u = ((a >> 5) * 2^26 + (b >> 6)) * 2^-53 with a, b the words 2 (i & 1), 2 (i & 1) + 1 of Philox4x32-10 on the counter
//   (i >> 1, c, d, stream_s) and the key (seed lo, seed hi): a function of the sample's stream id, not of its slot.
// Here w_k is formed as exp(alpha[i][k]) * exp(T[i][z][k]) and the c_k are added in state order.

#include "philox.h"

constexpr int SAMPLE_BLOCK = 256;      // draws of one workgroup: lane = draw
constexpr int SAMPLE_STAGE = 12;       // table elements a thread stages per step; S * S <= 12 * 256: S <= 55 (10 founders)

inline bool sample_table_in_lds(int S) { return S * S <= SAMPLE_STAGE * SAMPLE_BLOCK; }
// per buffer: the alpha column, its exp, and exp(T[i]) with rows S | 1 doubles apart; two buffers
inline size_t sample_lds_doubles(int S) { return 2 * (size_t)S + (sample_table_in_lds(S) ? (size_t)S * (S | 1) : 0); }
inline size_t sample_lds(int S) { return 2 * sample_lds_doubles(S) * sizeof(double); }

// 2 - |{a,b} n {c,d}| over multisets for every pair of states, states in combinations_with_replacement order
inline std::vector<uint8_t> sample_change_table(int H) {
    std::vector<std::pair<int, int>> st;
    for (int a = 0; a < H; ++a)
        for (int b = a; b < H; ++b) st.emplace_back(a, b);
    const size_t S = st.size();
    std::vector<uint8_t> tab(S * S);
    for (size_t p = 0; p < S; ++p)
        for (size_t q = 0; q < S; ++q) {
            const int a = st[p].first, b = st[p].second, c = st[q].first, d = st[q].second;
            int m = 0;
            if (a == c) m = 1 + (b == d);
            else if (a == d) m = 1 + (b == c);
            else m = (b == c) || (b == d);
            tab[p * S + q] = (uint8_t)(2 - m);
        }
    return tab;
}

// One workgroup per (block of 256 draws, chromosome, sample); the chain over the genes is sequential, and every step's
// alpha column and transition block are staged once for all the block's draws while the lanes work on the step before:
// a thread loads its share into registers, takes its draw's step, and only then takes the exp of what it loaded and
// stores it to the other LDS buffer - one barrier per step, one exp per table element per workgroup instead of per lane.
// Rows of the staged block are S | 1 doubles apart: at a step every lane reads column k of its own row z_{i+1}, lanes on
// one row read one address (a broadcast), lanes on rows r and r' land (r - r') * (S | 1) doubles apart, an odd multiple,
// so only rows 32 apart share a bank pair (ds_read_b64: 64 banks of 4 bytes, 32 lanes per group).
// TABLE_LDS = false (S > 55; S = 136: a block is 148 KB and does not fit twice): the lane reads the S doubles of its row
// through L2 and takes their exp itself; the alpha column is staged as before.
// States go out as bytes, cols[slot][gene][slab draw]: the lanes of a step write consecutive bytes
// (sample_transpose_kernel makes a draw's chromosome contiguous).  changes[slot][slab draw][chromosome] (nullable).
template <bool TABLE_LDS>
__global__ void __launch_bounds__(SAMPLE_BLOCK)
sample_paths_kernel(int S, int n_chrom, int64_t total_genes, int sample0, uint32_t draw0, int slab_draws,
                    const ChromDesc *__restrict__ chroms, const int32_t *__restrict__ order,
                    const double *__restrict__ alpha, const double *__restrict__ tprob,
                    const uint8_t *__restrict__ change_tab, const uint32_t *__restrict__ streams, uint32_t k0, uint32_t k1,
                    uint8_t *__restrict__ cols, int32_t *__restrict__ changes, unsigned long long *__restrict__ degenerate) {
    extern __shared__ double sample_buf[];
    const int tid = threadIdx.x;
    const int c = order[blockIdx.y];
    const ChromDesc cd = chroms[c];
    const int n = cd.n_genes;
    if (n < 1) return;
    const int slot = blockIdx.z;
    const int d_local = (int)blockIdx.x * SAMPLE_BLOCK + tid;
    const bool active = d_local < slab_draws;
    const uint32_t d = draw0 + (uint32_t)d_local, stream = streams[slot];
    const int LD = S | 1, SS = S * S;
    const size_t per = 2 * (size_t)S + (TABLE_LDS ? (size_t)S * LD : 0);
    const double *a_rows = alpha + ((int64_t)(sample0 + slot) * total_genes + cd.gene_off) * S;
    const double *T = tprob + cd.trans_off * SS;
    uint8_t *out = cols + ((int64_t)slot * total_genes + cd.gene_off) * slab_draws + d_local;

    double reg_a = 0.0, reg_t[TABLE_LDS ? SAMPLE_STAGE : 1];
    auto stage_load = [&](int i, bool table) {          // gene i's alpha column and T[i] into registers
        if (tid < S) reg_a = a_rows[(int64_t)i * S + tid];
        if (TABLE_LDS && table) {
            const double *blk = T + (int64_t)i * SS;
#pragma unroll
            for (int e = 0; e < SAMPLE_STAGE; ++e) {
                const int idx = tid + e * SAMPLE_BLOCK;
                if (idx < SS) reg_t[e] = blk[idx];
            }
        }
    };
    auto stage_store = [&](double *buf, bool table) {   // buf: [S] alpha, [S] exp(alpha), [S][LD] exp(T)
        if (tid < S) { buf[tid] = reg_a; buf[S + tid] = exp(reg_a); }
        if (TABLE_LDS && table) {
#pragma unroll
            for (int e = 0; e < SAMPLE_STAGE; ++e) {
                const int idx = tid + e * SAMPLE_BLOCK;
                if (idx < SS) {
                    const int r = idx / S, k = idx - r * S;
                    buf[2 * S + r * LD + k] = exp(reg_t[e]);
                }
            }
        }
    };

    stage_load(n - 1, false);
    stage_store(sample_buf, false);
    __syncthreads();
    uint32_t word[4] = {0u, 0u, 0u, 0u};
    int z_next = 0, n_changes = 0, parity = 0;
    for (int i = n - 1; i >= 0; --i) {
        const double *cur = sample_buf + parity * per;
        double *nxt = sample_buf + (parity ^ 1) * per;
        const bool more = i > 0, last = i == n - 1;
        if (more) stage_load(i - 1, true);               // T[i - 1]: i - 1 <= n - 2
        if (active) {
            if (last || (i & 1)) {                        // one block of four words serves genes 2 j + 1 and 2 j
                word[0] = (uint32_t)(i >> 1); word[1] = (uint32_t)c; word[2] = d; word[3] = stream;
                philox4x32_10(word, k0, k1);
            }
            const uint32_t wa = (i & 1) ? word[2] : word[0], wb = (i & 1) ? word[3] : word[1];
            const double u = ((double)(wa >> 5) * 67108864.0 + (double)(wb >> 6)) * (1.0 / 9007199254740992.0);
            const double *ea = cur + S;
            const double *row_lds = cur + 2 * S + z_next * LD;                    // TABLE_LDS, below the last gene
            const double *row_log = T + ((int64_t)i * S + z_next) * S;            // read below the last gene only
            auto weight = [&](int k) -> double {
                if (last) return ea[k];
                return ea[k] * (TABLE_LDS ? row_lds[k] : exp(row_log[k]));
            };
            double total = 0.0;
            for (int k = 0; k < S; ++k) total += weight(k);
            int z = -1;
            if (total > 0.0 && total <= DBL_MAX) {
                const double t = u * total;
                double run = 0.0;
                int last_pos = 0;
                for (int k = 0; k < S; ++k) {
                    const double w = weight(k);
                    run += w;
                    if (w > 0.0) last_pos = k;
                    if (z < 0 && run > t) z = k;
                }
                if (z < 0) z = last_pos;
            } else {
                double best = cur[0] + (last ? 0.0 : row_log[0]);
                z = 0;
                for (int k = 1; k < S; ++k) {
                    const double l = cur[k] + (last ? 0.0 : row_log[k]);
                    if (l > best) { best = l; z = k; }
                }
                atomicAdd(degenerate, 1ull);
            }
            out[(int64_t)i * slab_draws] = (uint8_t)z;
            if (!last) n_changes += change_tab[z_next * S + z];
            z_next = z;
        }
        if (more) stage_store(nxt, true);
        __syncthreads();
        parity ^= 1;
    }
    if (active && changes) changes[((int64_t)slot * slab_draws + d_local) * n_chrom + c] = n_changes;
}

// cols[slot][gene][slab draw] -> paths[slot][slab draw][gene]: 64 x 64 byte tiles through LDS, both sides coalesced
__global__ void __launch_bounds__(256)
sample_transpose_kernel(int64_t total_genes, int slab_draws, const uint8_t *__restrict__ cols, uint8_t *__restrict__ paths) {
    __shared__ uint8_t tile[64][65];
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int64_t g0 = (int64_t)blockIdx.x * 64;
    const int d0 = (int)blockIdx.y * 64;
    const uint8_t *in = cols + (int64_t)blockIdx.z * total_genes * slab_draws;
    uint8_t *out = paths + (int64_t)blockIdx.z * total_genes * slab_draws;
    for (int r = ty; r < 64; r += 4)
        if (g0 + r < total_genes && d0 + tx < slab_draws) tile[r][tx] = in[(g0 + r) * slab_draws + d0 + tx];
    __syncthreads();
    for (int r = ty; r < 64; r += 4)
        if (d0 + r < slab_draws && g0 + tx < total_genes) out[(int64_t)(d0 + r) * total_genes + g0 + tx] = tile[tx][r];
}
