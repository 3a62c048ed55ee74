#!/usr/bin/env python3
"""What the operators of the device tensor (gbrs_amd.tensor.DeviceTensor, gbrs_tensor_*) cost on the BASELINE configs[1]
sample (40M reads x 8 haplotypes x 120k isoforms, built in HBM by gbrs_amd.synth_torch and copied to the host once,
since gbrs_tensor_create takes host arrays).  Needs an MI355X; nothing here sets a threshold.

    timeout -k 10 900 python scripts/tensor_bench.py --out profiles/tensor_bench_40M.json

call_ms is a host clock around one blocking call (it ends in a stream synchronise), best and median of --steps calls
after one warm-up.  It includes what the call moves between host and device: the multiplier (8 R bytes for a read
vector, 8 R H for the reads x haplotypes matrix) and the result of a sum (8 R H bytes for sum(LOCUS)); host_bytes says
how much.  Kernel times come from a second run under the profiler, whose statistics file is merged in:

    rocprofv3 --kernel-trace --stats -f csv -d <dir> -- python scripts/tensor_bench.py --steps 1 --out <dir>/traced.json
    python scripts/tensor_bench.py --merge-kernel-stats <dir> --out profiles/tensor_bench_40M.json

kernel_ms is then the profiler's average per launch and kernel_GBps the bytes the operation has to move (entry_bytes per
stored entry, counted from the arrays the kernel reads and writes once) over it.  Without the merge they are absent:
not measured.
"""
import argparse
import csv
import glob
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# operation -> (kernel, bytes per stored entry the kernel must read and write once).  val 8 B read + 8 B written, the
# eliminated byte 1, the row id 4, an order's (lh, src) pair 8; a row pass reads val twice (sums, then the division).
KERNELS = {
    "reset": ("tensor_elementwise_kernel<0>", 8 + 1),
    "multiply_locus": ("tensor_elementwise_kernel<1>", 16 + 1),
    "multiply_read": ("tensor_elementwise_kernel<2>", 16 + 1 + 4),
    "multiply_read_hap": ("tensor_elementwise_kernel<3>", 16 + 1 + 4 + 8),
    "multiply_hap_locus": ("tensor_elementwise_kernel<4>", 16 + 1),
    "multiply_tensor": ("tensor_elementwise_kernel<5>", 24 + 1),
    "normalize_read": ("tensor_normalize_kernel<2>", 8 + 24 + 1),
    "normalize_locus": ("tensor_normalize_kernel<0>", 8 + 24 + 2),
    "normalize_group": ("tensor_normalize_kernel<3>", 8 + 24 + 2),
    "normalize_haplogroup": ("tensor_normalize_kernel<4>", 8 + 24 + 2),
    "normalize_haplotype": ("tensor_hap_sums_kernel<8,1>", 8 + 24 + 1),
    "sum_read": ("tensor_sum_reads_kernel", 8 + 4),
    "sum_locus": ("tensor_hap_sums_kernel<8,0>", 8 + 8 + 1),
}


def merge_kernel_stats(directory, path):
    res = json.load(open(path))
    rows = []
    for f in glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True):
        rows += list(csv.DictReader(open(f)))
    if not rows:
        raise SystemExit(f"no *kernel_stats.csv under {directory}")
    stats = {}
    for r in rows:
        name = r["Name"]
        for junk, to in (("void ", ""), ("(anonymous namespace)::", ""), ("(int)", ""), ("(bool)", ""), (".kd", ""),
                         (" ", ""), ("true", "1"), ("false", "0")):
            name = name.replace(junk, to)
        name = name.split("(")[0]
        stats[name] = dict(calls=int(r["Calls"]), average_ms=float(r["AverageNs"]) / 1e6, min_ms=float(r["MinNs"]) / 1e6,
                           max_ms=float(r["MaxNs"]) / 1e6)
    res["kernel_stats"] = {k: v for k, v in stats.items() if k.startswith("tensor_")}
    # a kernel's average is over every launch of the traced run: the warm-up, the timed call, the composed EM step
    for op, (kernel, per_entry) in KERNELS.items():
        if op in res["operations"] and kernel in stats:
            o = res["operations"][op]
            o["kernel"], o["kernel_ms"] = kernel, stats[kernel]["average_ms"]
            o["kernel_GBps"] = per_entry * res["entries"] / stats[kernel]["average_ms"] / 1e6
    json.dump(res, open(path, "w"), indent=1)
    print(json.dumps(res["kernel_stats"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--reads", type=int, default=40_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tensor_bench_40M.json"))
    ap.add_argument("--merge-kernel-stats", metavar="DIR")
    args = ap.parse_args()
    if args.merge_kernel_stats:
        return merge_kernel_stats(args.merge_kernel_stats, args.out)
    import numpy as np
    import torch
    from gbrs_amd import synth, synth_torch
    from gbrs_amd.alignment import AlignmentPropertyMatrix

    H, L = 8, 120_000
    prob = synth_torch.make_em_problem_device(args.reads, H, L, synth.SEED_BASE_EM + 1, "cuda:0")
    R, N = prob["R"], int(prob["N"])
    indptr = [t.cpu().numpy().view(np.uint32) for t in prob["indptr"]]
    indices = [t.cpu().numpy().view(np.uint32) for t in prob["indices"]]
    starts = np.asarray(prob["gene_starts"], dtype=np.int64)
    eff_len = prob["eff_len"].cpu().numpy()
    del prob
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    apm = AlignmentPropertyMatrix(shape=(L, H, R), indptr=indptr, indices=indices)
    apm.groups = [np.arange(a, b) for a, b in zip(starts, np.concatenate((starts[1:], [L])))]
    apm.num_groups = len(apm.groups)

    def used():
        torch.cuda.synchronize()
        return int(torch.cuda.mem_get_info()[1] - torch.cuda.mem_get_info()[0])

    def clock(fn, steps=None):
        fn()                                                # warm-up
        ms = []
        for _ in range(steps or args.steps):
            t0 = time.perf_counter()
            fn()
            ms.append((time.perf_counter() - t0) * 1e3)
        return dict(call_ms_best=min(ms), call_ms_median=statistics.median(ms))

    res = dict(workload=f"configs[1] sample: R={R} reads x H={H} x L={L} isoforms, N={N} entries, {len(starts)} genes",
               entries=N, reads=R, steps=args.steps, operations={})
    ops = res["operations"]
    base = used()
    t0 = time.perf_counter()
    t = apm.on_device()
    res["create_ms"] = (time.perf_counter() - t0) * 1e3
    res["handle_bytes"] = used() - base
    A = t.Axis
    t0 = time.perf_counter()
    t.normalize_reads(axis=A.READ)                          # builds the (row, gene, locus, haplotype) order
    res["first_row_pass_ms"] = (time.perf_counter() - t0) * 1e3
    res["handle_bytes_with_first_order"] = used() - base
    theta = t.sum(axis=A.READ) / eff_len
    t0 = time.perf_counter()
    t.normalize_reads(axis=A.HAPLOGROUP)                    # builds the (row, gene, haplotype, locus) order
    res["first_haplogroup_pass_ms"] = (time.perf_counter() - t0) * 1e3
    res["handle_bytes_with_both_orders"] = used() - base
    for key in ("handle_bytes", "handle_bytes_with_first_order", "handle_bytes_with_both_orders"):
        res[key + "_per_entry"] = res[key] / N

    m_l, m_r, m_rh, m_hl = np.full(L, 1.25), np.full(R, 1.25), np.full((R, H), 1.25), np.full((H, L), 1.25)

    def timed(name, fn, host_bytes=0):
        t.reset()
        ops[name] = dict(clock(fn), host_bytes=host_bytes, entry_bytes=KERNELS[name][1])

    timed("reset", t.reset)
    timed("multiply_locus", lambda: t.multiply(m_l, axis=1), m_l.nbytes)
    timed("multiply_read", lambda: t.multiply(m_r, axis=2), m_r.nbytes)
    timed("multiply_read_hap", lambda: t.multiply(m_rh, axis=0), m_rh.nbytes)
    timed("multiply_hap_locus", lambda: t.multiply(m_hl, axis=2), m_hl.nbytes)
    del m_r, m_rh
    c = t.copy()
    res["copy_bytes"] = used() - base - res["handle_bytes_with_both_orders"]
    timed("multiply_tensor", lambda: t.multiply(c))
    c.close()
    ops["copy"] = clock(lambda: t.copy().close())
    for name, axis in (("normalize_read", A.READ), ("normalize_haplotype", A.HAPLOTYPE), ("normalize_locus", A.LOCUS),
                       ("normalize_group", A.GROUP), ("normalize_haplogroup", A.HAPLOGROUP)):
        timed(name, lambda axis=axis: t.normalize_reads(axis=axis))
    timed("sum_read", lambda: t.sum(axis=A.READ), 8 * H * L)
    timed("sum_locus", lambda: t.sum(axis=A.LOCUS), 8 * R * H)

    # the reference's Model-2 E-step (EMfactory.py:176-191) and M-step from the operators
    def model2_step():
        nonlocal theta
        t.reset()
        t.multiply(theta, axis=A.READ)
        t.normalize_reads(axis=A.LOCUS)
        t.multiply(theta.sum(axis=0), axis=A.HAPLOTYPE)
        t.normalize_reads(axis=A.GROUP)
        gene_tot = np.add.reduceat(theta.sum(axis=0), starts)
        t.multiply(np.repeat(gene_tot, np.diff(np.concatenate((starts, [L])))), axis=A.HAPLOTYPE)
        t.normalize_reads(axis=A.READ)
        theta = t.sum(axis=A.READ) / eff_len
    ops["model2_em_step_composed"] = clock(model2_step)
    res["live_entries_after_model2"] = t.nnz()
    t.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(res, open(args.out, "w"), indent=1)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
