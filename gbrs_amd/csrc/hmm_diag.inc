// Diagnostics of the last run (gbrs_hmm_diagnostics, gbrs_hmm_pair_posterior; DESIGN.md §23): the pair posteriors of
// neighbouring genes reduced to the expected founder changes and the switch probability of every interval, and per gene
// the error LOD and the most likely diplotype.  Reads what hmm_make_logs leaves - alpha, beta ([sample][gene][S], logs) -
// with eprob, gamma and the handle's log tables T[i][to][from] in their uploaded order.  Included by hmm_passes.hip inside
// namespace gbrs.
//
// Interval i -> i+1 of sample s on chromosome c (k the state at gene i, j at gene i+1):
//   lx[k][j] = alpha[i][k] + T[i][j][k] + E[i+1][j] + beta[i+1][j],  m = max lx,  x = exp(lx - m) (0 where lx is -inf)
//   xi[k][j] = x / sum x,  xo = sum x * change[k][j] / sum x,  pswitch = sum_{k != j} x / sum x
// Gene i:  errlod = (lse(iv + E[i]) - (lse(alpha + beta) - lse((alpha - E) + beta))) / ln 10, an entry whose alpha is -inf
//   carrying weight 0;  maxmarg = the first argmax of gamma[i], maxprob its value.

constexpr int DIAG_BLOCK = 256;            // four wavefronts; a wavefront owns one sample of an interval at a time
constexpr int DIAG_WAVES = DIAG_BLOCK / 64;
constexpr int DIAG_RUN = 8;                // consecutive genes of one workgroup
constexpr int DIAG_LDS_STATES = 55;        // a table block is staged in LDS up to this many states (24 KB), as in hmm_sample.inc

inline bool diag_table_in_lds(int S) { return S <= DIAG_LDS_STATES; }
inline size_t diag_pair_lds(int S) {       // per wavefront the alpha column and E + beta of the next gene; the table block
    return ((size_t)DIAG_WAVES * 2 * S + (diag_table_in_lds(S) ? (size_t)S * S : 0)) * sizeof(double);
}

__device__ __forceinline__ double diag_wave_max_all(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off, WAVE));
    return v;
}

// lse over the S entries a wavefront's lanes hold strided (k = lane, lane + 64, ..): max + log sum exp(v - max), -inf
// entries carrying weight 0.  `term(k)` gives entry k.  Same value in every lane.
template <typename F>
__device__ __forceinline__ double diag_wave_lse(int S, int lane, F term) {
    double m = -INFINITY;
    for (int k = lane; k < S; k += WAVE) m = fmax(m, term(k));
    m = diag_wave_max_all(m);
    double sum = 0.0;
    for (int k = lane; k < S; k += WAVE) {
        const double v = term(k);
        sum += v == -INFINITY ? 0.0 : exp(v - m);
    }
    return m + log(wave_sum_all(sum));
}

// One workgroup per (run of DIAG_RUN consecutive genes, slab of samples).  Gene g that is not the last of its chromosome
// stands for the interval g -> g + 1; the last gene's slot gets 0.0.  T[i] is read once per workgroup into LDS
// (TABLE_LDS) and serves every sample of the slab; above 55 states a block does not fit beside a second workgroup and
// the lanes read it through L2, consecutive lanes consecutive elements.  A wavefront takes the slab's samples w, w + 4,
// ..: its lanes walk the S * S elements in table order (idx = j * S + k), first for the maximum, then for the three sums
// (the second walk recomputes lx: three additions against one exp), reduced by butterflies in a fixed order - a value
// depends on neither the slab nor the run it was computed in.
// XI: the launch covers one (sample, chromosome) and also writes xi[i][k][j]; gene_begin is then the chromosome's first gene.
template <bool TABLE_LDS, bool XI>
__global__ void __launch_bounds__(DIAG_BLOCK)
diag_pair_kernel(int S, int n_chrom, int64_t total_genes, int64_t gene_begin, int64_t gene_end, int sample0, int n_samples,
                 int slab, const ChromDesc *__restrict__ chroms, const double *__restrict__ alpha,
                 const double *__restrict__ beta, const double *__restrict__ eprob, const double *__restrict__ tprob,
                 const uint8_t *__restrict__ change_tab, double *__restrict__ xo, double *__restrict__ pswitch,
                 double *__restrict__ xi) {
    extern __shared__ double diag_buf[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int SS = S * S;
    double *col_a = diag_buf + (size_t)wave * 2 * S;       // alpha[i][k]
    double *col_eb = col_a + S;                            // E[i+1][j] + beta[i+1][j]
    double *tab = diag_buf + (size_t)DIAG_WAVES * 2 * S;   // T[i], TABLE_LDS only
    const int64_t g_lo = gene_begin + (int64_t)blockIdx.x * DIAG_RUN;
    const int64_t g_hi = min(g_lo + DIAG_RUN, gene_end);
    const int slot_lo = (int)blockIdx.y * slab, slot_hi = min(slot_lo + slab, n_samples);
    int c = 0;
    for (int64_t g = g_lo; g < g_hi; ++g) {
        while (c + 1 < n_chrom && (chroms[c].n_genes == 0 || g >= chroms[c].gene_off + chroms[c].n_genes)) ++c;
        const ChromDesc cd = chroms[c];
        const int i = (int)(g - cd.gene_off);
        if (i < 0 || i >= cd.n_genes) continue;            // not reached: the chromosomes tile [0, total_genes)
        if (i == cd.n_genes - 1) {                         // no interval leaves a chromosome's last gene
            for (int slot = slot_lo + tid; slot < slot_hi; slot += DIAG_BLOCK) {
                if (xo) xo[(int64_t)slot * total_genes + g] = 0.0;
                if (pswitch) pswitch[(int64_t)slot * total_genes + g] = 0.0;
            }
            continue;
        }
        const double *T = tprob + (cd.trans_off + i) * (int64_t)SS;
        if (TABLE_LDS) {
            __syncthreads();                               // the walks of the gene before are done with `tab`
            for (int idx = tid; idx < SS; idx += DIAG_BLOCK) tab[idx] = T[idx];
            __syncthreads();
        }
        for (int slot = slot_lo + wave; slot < slot_hi; slot += DIAG_WAVES) {
            const int64_t row = ((int64_t)(sample0 + slot) * total_genes + g) * S;
            for (int k = lane; k < S; k += WAVE) {
                col_a[k] = alpha[row + k];
                col_eb[k] = eprob[row + S + k] + beta[row + S + k];
            }
            // the wavefront's own LDS rows: written and read by this wavefront alone, in program order
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            auto walk = [&](auto visit) {                  // visit(idx, j, k, lx) over this lane's elements, in table order
                int j = 0, k = lane;
                for (int idx = lane; idx < SS; idx += WAVE) {
                    while (k >= S) { k -= S; ++j; }
                    visit(idx, j, k, ((col_a[k] + (TABLE_LDS ? tab[idx] : T[idx])) + col_eb[j]));
                    k += WAVE;
                }
            };
            double m = -INFINITY;
            walk([&](int, int, int, double lx) { m = fmax(m, lx); });
            m = diag_wave_max_all(m);
            double sum = 0.0, sum_ch = 0.0, sum_off = 0.0;
            walk([&](int idx, int j, int k, double lx) {
                const double x = lx == -INFINITY ? 0.0 : exp(lx - m);
                sum += x;
                sum_ch += x * (double)change_tab[idx];     // the change table is symmetric: [j][k] = [k][j]
                if (j != k) sum_off += x;
            });
            sum = wave_sum_all(sum);
            sum_ch = wave_sum_all(sum_ch);
            sum_off = wave_sum_all(sum_off);
            if (lane == 0) {
                if (xo) xo[(int64_t)slot * total_genes + g] = sum_ch / sum;
                if (pswitch) pswitch[(int64_t)slot * total_genes + g] = sum_off / sum;
            }
            if (XI) {
                double *out = xi + (int64_t)i * SS;
                walk([&](int, int j, int k, double lx) {
                    out[k * S + j] = (lx == -INFINITY ? 0.0 : exp(lx - m)) / sum;
                });
            }
            __builtin_amdgcn_wave_barrier();               // the next sample overwrites the rows
        }
    }
}

// One wavefront per (sample, gene) row; the lanes hold the states strided.
__global__ void __launch_bounds__(DIAG_BLOCK)
diag_gene_kernel(int S, int64_t total_genes, int sample0, int64_t rows, const double *__restrict__ init_vec,
                 const double *__restrict__ alpha, const double *__restrict__ beta, const double *__restrict__ eprob,
                 const double *__restrict__ gamma, double *__restrict__ errlod, double *__restrict__ maxprob,
                 int32_t *__restrict__ maxmarg) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * DIAG_WAVES + (threadIdx.x >> 6);     // slot * total_genes + gene
    if (r >= rows) return;
    const int64_t base = ((int64_t)sample0 * total_genes + r) * S;
    if (errlod) {
        const double *a = alpha + base, *b = beta + base, *e = eprob + base;
        const double prior = diag_wave_lse(S, lane, [&](int k) { return init_vec[k] + e[k]; });
        const double with = diag_wave_lse(S, lane, [&](int k) { return a[k] + b[k]; });
        const double without = diag_wave_lse(S, lane, [&](int k) {
            return a[k] == -INFINITY ? -INFINITY : (a[k] - e[k]) + b[k];
        });
        if (lane == 0) errlod[r] = (prior - (with - without)) / 2.302585092994045684;
    }
    if (maxprob || maxmarg) {
        const double *p = gamma + base;
        double best = -INFINITY;
        int at = S;                                        // no entry above -inf (NaN rows): index 0 below
        for (int k = lane; k < S; k += WAVE)
            if (p[k] > best) { best = p[k]; at = k; }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const double v = __shfl_xor(best, off, WAVE);
            const int w = __shfl_xor(at, off, WAVE);
            if (v > best || (v == best && w < at)) { best = v; at = w; }
        }
        if (lane == 0) {
            if (at >= S) { at = 0; best = p[0]; }
            if (maxprob) maxprob[r] = best;
            if (maxmarg) maxmarg[r] = at;
        }
    }
}
