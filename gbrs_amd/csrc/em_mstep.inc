// M-step kernels for a power-of-two haplotype count (included by em.hip): the element-parallel M-step of the sharded
// path and of prepare, and the fused gather + M-step of a single-GPU step.  The haplotype count is a template argument,
// so the locus of an element is a shift, a thread owns two adjacent haplotypes of a locus and moves them with one 16-byte
// access, and a locus's totals are an in-lane add and compile-time DPP steps over the H / 2 lanes that hold it.

template <int H> struct MstepRow {
    static_assert(H == 1 || H == 2 || H == 4 || H == 8 || H == 16 || H == 32, "a power of two up to 32");
    static constexpr int P = H > 1 ? 2 : 1;          // haplotypes a thread owns: one 16-byte access (8 bytes at H = 1)
    static constexpr int LANES = H / P;              // adjacent lanes that hold one locus
    static constexpr int LANE_SHIFT = LANES == 1 ? 0 : LANES == 2 ? 1 : LANES == 4 ? 2 : LANES == 8 ? 3 : 4;
    static constexpr int H_SHIFT = LANE_SHIFT + P - 1;
};
template <int P> struct alignas(8 * P) HapVec { double v[P]; };

template <int P> __device__ __forceinline__ HapVec<P> hap_load(const double *p) {
    return *reinterpret_cast<const HapVec<P> *>(p);
}
template <int P> __device__ __forceinline__ void hap_store(double *p, const HapVec<P> &x) {
    *reinterpret_cast<HapVec<P> *>(p) = x;
}
template <int P> __device__ __forceinline__ HapVec<P> hap_fill(double x) {
    HapVec<P> r;
#pragma unroll
    for (int j = 0; j < P; ++j) r.v[j] = x;
    return r;
}

// Keeps a loaded value where it was loaded.  Without it the compiler moves the loads of a thread's first element behind
// the test of its class byte: a second, dependent round trip.
template <int P> __device__ __forceinline__ void hap_pin(HapVec<P> &x) {
#pragma unroll
    for (int j = 0; j < P; ++j) asm volatile("" : "+v"(x.v[j]));
}

template <int CTRL> __device__ __forceinline__ double mstep_dpp(double x) {
    int lo = __double2loint(x), hi = __double2hiint(x);
    lo = __builtin_amdgcn_update_dpp(lo, lo, CTRL, 0xf, 0xf, false);
    hi = __builtin_amdgcn_update_dpp(hi, hi, CTRL, 0xf, 0xf, false);
    return __hiloint2double(hi, lo);
}

// The sum of x over the haplotypes of the locus, in every lane that holds it.  The pairing tree is that of xor steps 1, 2,
// 4, ... over one haplotype per lane: (h0 + h1) in the lane, then pairs of pairs.  After a step all lanes of a group hold
// the same value, so the mirrored half (row_half_mirror, row_mirror) gives what the xor 4 / xor 8 lane would.
// Call it with every lane of the wavefront active.
template <int H> __device__ __forceinline__ double locus_total(const HapVec<MstepRow<H>::P> &x) {
    constexpr int LANES = MstepRow<H>::LANES;
    double s = x.v[0];
    if (MstepRow<H>::P == 2) s += x.v[MstepRow<H>::P - 1];
    if (LANES >= 2) s += mstep_dpp<0xB1>(s);         // quad_perm:[1,0,3,2]
    if (LANES >= 4) s += mstep_dpp<0x4E>(s);         // quad_perm:[2,3,0,1]
    if (LANES >= 8) s += mstep_dpp<0x141>(s);        // row_half_mirror
    if (LANES >= 16) s += mstep_dpp<0x140>(s);       // row_mirror
    return s;
}

// One thread's haplotypes of a locus row: c = theta * A, theta' = c / len, and the locus's totals of theta and theta'.
// A lane that has no row passes zeros (and ones for len) and adds nothing.
template <int H>
__device__ __forceinline__ void mstep_row(const HapVec<MstepRow<H>::P> &t, const HapVec<MstepRow<H>::P> &a,
                                          const HapVec<MstepRow<H>::P> &len, bool has_len, HapVec<MstepRow<H>::P> &c,
                                          HapVec<MstepRow<H>::P> &tn, double &tot_prev, double &tot_new) {
#pragma unroll
    for (int j = 0; j < MstepRow<H>::P; ++j) {
        c.v[j] = t.v[j] * a.v[j];
        tn.v[j] = has_len ? c.v[j] / len.v[j] : c.v[j];
    }
    tot_prev = locus_total<H>(t);
    tot_new = locus_total<H>(tn);
}
template <int P> __device__ __forceinline__ double hap_sum(const HapVec<P> &x) {
    double s = x.v[0];
    if (P == 2) s += x.v[P - 1];
    return s;
}

// Element-parallel M-step for H a power of two: one thread per pair of haplotypes of a locus, the lanes of a locus
// adjacent, so every access is a coalesced 16-byte stream.  A comes from `acc` (tile epilogues for single-tile loci,
// gather_kernel for the rest; loci without any read stay 0).  One block sum per workgroup of theta before / after.
template <int MODE, int H>
__global__ void __launch_bounds__(RED_THREADS)
mstep_elem_kernel(uint32_t L, double *__restrict__ theta, const double *__restrict__ acc,
                  const double *__restrict__ acc_extra, const double *__restrict__ eff_len,
                  double *__restrict__ counts, double *__restrict__ tot_prev, double *__restrict__ tot_new,
                  double *__restrict__ msums, uint32_t cap, const EmScalars *__restrict__ sc) {
    using R = MstepRow<H>;
    using Vec = HapVec<R::P>;
    __shared__ double lds[16];
    if (MODE == 0 && sc->stop) return;
    const uint64_t npair = (uint64_t)L << R::LANE_SHIFT;
    const uint64_t p = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool ok = p < npair;
    const uint64_t pc = ok ? p : npair - 1;             // (the lanes past the end read the last row again and drop it)
    const size_t i = (size_t)pc * R::P;
    Vec a = hap_load<R::P>(acc + i), t = hap_fill<R::P>(1.0), len = hap_fill<R::P>(1.0);
    if (MODE == 0) t = hap_load<R::P>(theta + i);
    if (acc_extra) {
        const Vec x = hap_load<R::P>(acc_extra + i);
#pragma unroll
        for (int j = 0; j < R::P; ++j) a.v[j] += x.v[j];
    }
    if (eff_len) len = hap_load<R::P>(eff_len + i);
    if (!ok) {
        t = hap_fill<R::P>(0.0);
        a = hap_fill<R::P>(0.0);
        len = hap_fill<R::P>(1.0);
    }
    Vec c, tn;
    double tp, tq;
    mstep_row<H>(t, a, len, eff_len != nullptr, c, tn, tp, tq);
    if (ok) {
        hap_store<R::P>(counts + i, c);
        hap_store<R::P>(theta + i, tn);
        if ((pc & (R::LANES - 1)) == 0) {
            const uint32_t l = (uint32_t)(pc >> R::LANE_SHIFT);
            tot_prev[l] = tp;
            tot_new[l] = tq;
        }
    }
    const double sa = block_sum(hap_sum<R::P>(t), lds);
    const double sb = block_sum(hap_sum<R::P>(tn), lds);
    if (threadIdx.x == 0) {                 // one slot per workgroup: no atomics, and a fixed summation order
        msums[blockIdx.x] = sa;
        msums[cap + blockIdx.x] = sb;
    }
}

// Gather + M-step in one launch (tile layout, H a power of two, single GPU): an element of a locus
// with at most one slot takes A straight from `acc` (written by the tile epilogue), a locus with a
// few slots sums them in place, and the loci with many slots get one workgroup each (the leading
// workgroups), which reduces the slots in fixed order and applies the M-step to that locus itself.
// No intermediate A vector is written for the gathered loci and there is one launch less per step.
//
// Round 3: the launch was ~13 us of a ~115 us iteration and none of it was bandwidth - it is the number of
// DEPENDENT global loads on its longest path (a round trip is ~0.7 us): stop flag -> locus list -> slot_ptr ->
// four slot rows at a time -> ... .  Now every path is two round trips: (1) the stop flag, the (locus, first row,
// end row) record of a heavy / light locus, or class, theta, A and length of a plain element, all in flight
// together; (2) all the slot rows of the locus at once (a light locus has at most HEAVY_SLOTS of them; a heavy
// workgroup takes 16 rows per thread and round).  The stop flag only guards the stores.
//
// H, "the long rows' sums are in acc_extra" and "the handle has lengths" are template arguments: with the nullable
// pointers tested at run time the compiler put a wait in front of every element's optional loads, so a thread of the
// elementwise part made MSTEP_EPT dependent round trips with a 64-bit division between them.  Now all loads of a thread
// are issued (indices clamped, not branched on) before the first wait.
#ifndef GBRS_MSTEP_EPT
#define GBRS_MSTEP_EPT 2
#endif
constexpr int MSTEP_EPT = GBRS_MSTEP_EPT;       // 16-byte pairs per thread of the elementwise workgroups (measured: profiles/mstep_rows.txt)
constexpr int HEAVY_ROWS = 16;     // slot rows a thread of a heavy workgroup has in flight
template <int H, bool EXTRA, bool LEN>
__global__ void __launch_bounds__(RED_THREADS)
mstep_gather_kernel(uint32_t L, uint32_t heavy_blocks, uint32_t light_blocks, uint32_t n_light,
                    const uint32_t *__restrict__ heavy_range, const uint32_t *__restrict__ light_range,
                    const uint8_t *__restrict__ locus_class,
                    const double *__restrict__ slot_sums, const double *__restrict__ acc,
                    const double *__restrict__ acc_extra, double *__restrict__ theta,
                    const double *__restrict__ eff_len, double *__restrict__ tot_prev,
                    double *__restrict__ tot_new, double *__restrict__ msums, uint32_t cap,
                    const EmScalars *__restrict__ sc) {
    using R = MstepRow<H>;
    using Vec = HapVec<R::P>;
    constexpr uint32_t HP = H;          // the fused route takes powers of two only
    __shared__ double lds[16];
    __shared__ double heavy_part[RED_THREADS / 64][16];
    const int stop = sc->stop;          // scalar load, in flight beside the vector loads below; looked at before the stores
    double t = 0.0, tn = 0.0;
    if (blockIdx.x < heavy_blocks) {
        // one workgroup per many-slot locus: the largest loci of a deep sample have hundreds of slots whose rows
        // were written by tiles all over the chip a moment ago
        const uint32_t l = heavy_range[3 * blockIdx.x], k0 = heavy_range[3 * blockIdx.x + 1], k1 = heavy_range[3 * blockIdx.x + 2];
        const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
        const uint32_t h = threadIdx.x & (HP - 1), sub = threadIdx.x / HP, nsub = blockDim.x / HP;
        const size_t il = (size_t)l * H + h;
        const double t_old = theta[il], ax = EXTRA ? acc_extra[il] : 0.0, ln = LEN ? eff_len[il] : 1.0;
        double a = 0.0;
        for (uint32_t k = k0 + sub; k < k1; k += HEAVY_ROWS * nsub) {          // fixed order: rounds, then rows of a round
            double r[HEAVY_ROWS];
#pragma unroll
            for (int m = 0; m < HEAVY_ROWS; ++m) {
                const uint32_t km = k + (uint32_t)m * nsub;
                r[m] = km < k1 ? slot_sums[(size_t)km * H + h] : 0.0;
            }
#pragma unroll
            for (int w = 1; w < HEAVY_ROWS; w <<= 1)
#pragma unroll
                for (int m = 0; m + w < HEAVY_ROWS; m += 2 * w) r[m] += r[m + w];
            a += r[0];
        }
#pragma unroll
        for (uint32_t off = HP; off < 64; off <<= 1) a += __shfl_xor(a, off, WAVE);
        if (lane < (int)HP) heavy_part[wv][lane] = a;        // the wavefronts' partial sums, added in a fixed order
        __syncthreads();
        if (wv == 0) {
            a = 0.0;
            if (lane < (int)HP)
                for (uint32_t w2 = 0; w2 < blockDim.x / 64; ++w2) a += heavy_part[w2][lane];
            if (lane < (int)HP) {
                t = t_old;
                const double c = t * (a + ax);
                tn = LEN ? c / ln : c;
                if (!stop) theta[il] = tn;             // (the expected counts are theta' * len: made when asked for)
            }
            double tp = t, tq = tn;                       // lanes 0 .. H-1 hold the locus, the others 0
#pragma unroll
            for (uint32_t off = 1; off < HP; off <<= 1) {
                tp += __shfl_xor(tp, off, WAVE);
                tq += __shfl_xor(tq, off, WAVE);
            }
            if (lane == 0 && !stop) {
                tot_prev[l] = tp;
                tot_new[l] = tq;
            }
        }
    } else if (blockIdx.x < heavy_blocks + light_blocks) {
        // one thread per (light locus, pair of haplotypes): the locus's 2..HEAVY_SLOTS slot rows all at once, added in
        // slot order onto the long rows' sum
        const uint32_t i = (blockIdx.x - heavy_blocks) * blockDim.x + threadIdx.x;
        const bool live = i < (n_light << R::LANE_SHIFT);
        const uint32_t li = live ? i >> R::LANE_SHIFT : 0, h = (i & (R::LANES - 1)) * R::P;
        const uint32_t l = light_range[3 * li], k0 = light_range[3 * li + 1], k1 = light_range[3 * li + 2];
        const size_t il = ((size_t)l << R::H_SHIFT) + h;
        Vec t_old = hap_load<R::P>(theta + il), a = hap_fill<R::P>(0.0), ln = hap_fill<R::P>(1.0);
        if (EXTRA) a = hap_load<R::P>(acc_extra + il);
        if (LEN) ln = hap_load<R::P>(eff_len + il);
        Vec r[HEAVY_SLOTS];
#pragma unroll
        for (int m = 0; m < HEAVY_SLOTS; ++m)
            r[m] = k0 + m < k1 ? hap_load<R::P>(slot_sums + (((size_t)(k0 + m)) << R::H_SHIFT) + h) : hap_fill<R::P>(0.0);
#pragma unroll
        for (int m = 0; m < HEAVY_SLOTS; ++m)
#pragma unroll
            for (int j = 0; j < R::P; ++j) a.v[j] += r[m].v[j];
        if (!live) {
            t_old = hap_fill<R::P>(0.0);
            a = hap_fill<R::P>(0.0);
            ln = hap_fill<R::P>(1.0);
        }
        Vec c, tnew;
        double tp, tq;                                    // the lanes of a locus are adjacent
        mstep_row<H>(t_old, a, ln, LEN, c, tnew, tp, tq);
        if (live && !stop) {
            hap_store<R::P>(theta + il, tnew);
            if (h == 0) {
                tot_prev[l] = tp;
                tot_new[l] = tq;
            }
        }
        t = hap_sum<R::P>(t_old);
        tn = hap_sum<R::P>(tnew);
    } else {
        // MSTEP_EPT pairs per thread of the loci with at most one slot: class, theta, A and length of all of them in one
        // batch of loads, no second round trip
        const uint32_t npair = L << R::LANE_SHIFT;
        const uint32_t p0 = (blockIdx.x - heavy_blocks - light_blocks) * (MSTEP_EPT * blockDim.x) + threadIdx.x;
        uint32_t cls[MSTEP_EPT];
        Vec av[MSTEP_EPT], xv[MSTEP_EPT], tv[MSTEP_EPT], lv[MSTEP_EPT];
#pragma unroll
        for (int e = 0; e < MSTEP_EPT; ++e) {
            const uint32_t p = p0 + (uint32_t)e * blockDim.x;
            const uint32_t pc = p < npair ? p : npair - 1;    // (past the end: the last row again, dropped below)
            const size_t i = (size_t)pc * R::P;
            cls[e] = locus_class[pc >> R::LANE_SHIFT];
            tv[e] = hap_load<R::P>(theta + i);
            av[e] = hap_load<R::P>(acc + i);                  // one slot: stored by its tile; none: stays 0
            if (EXTRA) xv[e] = hap_load<R::P>(acc_extra + i);
            if (LEN) lv[e] = hap_load<R::P>(eff_len + i);
        }
#pragma unroll
        for (int e = 0; e < MSTEP_EPT; ++e) {
            hap_pin<R::P>(tv[e]);
            hap_pin<R::P>(av[e]);
            if (EXTRA) hap_pin<R::P>(xv[e]);
            if (LEN) hap_pin<R::P>(lv[e]);
        }
#pragma unroll
        for (int e = 0; e < MSTEP_EPT; ++e) {
            const uint32_t p = p0 + (uint32_t)e * blockDim.x;
            const bool mine = p < npair && cls[e] < 2;        // classes 2 and 3: the workgroups above
            Vec te, ae, le;                                   // (selects, not a branch: a branch takes the loads with it)
#pragma unroll
            for (int j = 0; j < R::P; ++j) {
                double aj = av[e].v[j];
                if (EXTRA) aj += xv[e].v[j];
                te.v[j] = mine ? tv[e].v[j] : 0.0;
                ae.v[j] = mine ? aj : 0.0;
                le.v[j] = LEN && mine ? lv[e].v[j] : 1.0;
            }
            Vec c, tne;
            double tp, tq;                                // the lanes of a locus are adjacent, same class
            mstep_row<H>(te, ae, le, LEN, c, tne, tp, tq);
            if (mine && !stop) {
                hap_store<R::P>(theta + (size_t)p * R::P, tne);
                if ((p & (R::LANES - 1)) == 0) {
                    tot_prev[p >> R::LANE_SHIFT] = tp;
                    tot_new[p >> R::LANE_SHIFT] = tq;
                }
            }
            t += hap_sum<R::P>(te);
            tn += hap_sum<R::P>(tne);
        }
    }
    const double a = block_sum(t, lds);
    const double b = block_sum(tn, lds);
    if (threadIdx.x == 0 && !stop) {
        msums[blockIdx.x] = a;
        msums[cap + blockIdx.x] = b;
    }
}
