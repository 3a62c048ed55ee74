#!/usr/bin/env python3
"""The match pass (`gbrs reconstruct --match-panel`) at DO size, against the host route.

    python scripts/match_bench.py [--samples 1,64,256] [--panels 64,512] [--grid-points 64000] [--runs 3] [--out profiles/match_bench.json]

Inputs: the DO-sized synthetic genome of scripts/grid_bench.py (synth.make_hmm_problem(H=8): 20 chromosomes, 40,000 genes),
gene positions drawn per chromosome, --grid-points markers spread evenly over the chromosomes, samples drawn by that
script's recipe, and panels of random dosages (rows that add up to 1).  Everything stays in this process: one handle, one
run per sample count, one upload per panel size.  Recorded per (panel entries, samples):

  pass_ms            device time of the match pass's own kernels from events (gbrs_hmm_match_info), the second of two calls
                     on dosages that gbrs_hmm_grid left on the device
  wall_after_grid_ms host clock around hmm.match() - kernels, synchronise and the two copies out - on those dosages, best of --runs
  wall_alone_ms      the same when the pass has to make the dosages first (its own launch of the grid kernel), best of --runs
  flops, tflops      2 n M K over pass_ms, K = grid points x founders
  bytes, hbm_floor_ms, share_of_hbm_floor
                     what the pass must move at least - both operands once and the outputs - and the time that takes at the
                     chip's 8 TB/s; the f64 matrix pipe's bound (78.6 TFLOP/s: 2048 FLOP per 64 cycles and SIMD) is given
                     beside it, and the larger of the two is the floor

  host route, at every (panel entries, samples) asked for with --host (default 512x64): hmm.grid()'s dosages copied to the
  host and A_c @ B_c.T in numpy per chromosome on this job's CPUs, the panel already in memory as one contiguous matrix per
  chromosome; best of --runs.

The one condition of the change is checked at the end: at 64 samples x 512 entries wall_alone_ms - the pass with its own
grid launch and its copies out - is below the host route's time."""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
HBM_BYTES_PER_S = 8.0e12
F64_MFMA_FLOPS = 256 * 4 * 2048 / 64 * 2.4e9


def problem(grid_points, n_samples):
    from gbrs_amd import synth
    prob = synth.make_hmm_problem(H=8)
    rng = np.random.default_rng(21)
    per = grid_points // len(prob.chroms)
    where, grid = [], []
    for k, c in enumerate(prob.chroms):
        where.append(np.sort(rng.uniform(3.0, 100.0, size=len(prob.gene_ids[c]))))
        grid.append(np.linspace(0.0, 101.0, per + (grid_points - per * len(prob.chroms) if k == 0 else 0)))
    expr = []
    for c in prob.chroms:
        n = len(prob.gene_ids[c])
        e = rng.gamma(1.0, 5.0, size=(n_samples, n, 8)) * (rng.random((n_samples, n, 8)) < 0.5)
        e[0] = np.array([prob.expr[g] for g in prob.gene_ids[c]])
        expr.append(np.round(e, 3))
    return prob, where, grid, expr


def best_of(runs, call):
    times = []
    for _ in range(runs):
        t0 = time.perf_counter()
        call()
        times.append(time.perf_counter() - t0)
    return min(times) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--samples", default="1,64,256")
    ap.add_argument("--panels", default="64,512")
    ap.add_argument("--host", default="512x64", help="comma list of <entries>x<samples> at which the host route is timed")
    ap.add_argument("--grid-points", type=int, default=64_000)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "match_bench.json"))
    a = ap.parse_args()
    counts = [int(x) for x in a.samples.split(",") if x]
    panels = [int(x) for x in a.panels.split(",") if x]
    host_at = {tuple(int(y) for y in x.split("x")) for x in a.host.split(",") if x}
    from gbrs_amd.hmm import DiplotypeHMM
    t0 = time.perf_counter()
    prob, where, grid, expr = problem(a.grid_points, max(counts))
    H, chroms = 8, prob.chroms
    points = [len(g) for g in grid]
    offsets = np.concatenate(([0], np.cumsum(points)[:-1]))
    P, K = sum(points), sum(points) * H
    rng = np.random.default_rng(22)
    entries = []
    for _ in range(max(panels)):
        b = rng.random((P, H))
        entries.append(b / b.sum(axis=1, keepdims=True))
    result = dict(genes=prob.num_genes, grid_points=P, founders=H, make_inputs_s=round(time.perf_counter() - t0, 2),
                  cpus=os.environ.get("OMP_NUM_THREADS", "not set"), hbm_peak_tb_s=HBM_BYTES_PER_S / 1e12,
                  f64_mfma_peak_tflops=round(F64_MFMA_FLOPS / 1e12, 1), passes={}, host_route={})
    hmm = DiplotypeHMM(H, chroms, [len(prob.gene_ids[c]) for c in chroms], [prob.tprob[c] for c in chroms])
    ha = [np.array([g in prob.avecs for g in prob.gene_ids[c]], dtype=np.uint8) for c in chroms]
    av = [np.array([prob.avecs.get(g, np.zeros((H, H))) for g in prob.gene_ids[c]]) for c in chroms]
    hmm.set_grid(where, grid)
    first = True
    for M in panels:
        t0 = time.perf_counter()
        hmm.set_panel(entries[:M])
        upload_s = time.perf_counter() - t0
        by_chrom = None
        for n in counts:
            rows = [e[:n] for e in expr]
            if first:
                hmm.set_expression(rows, av, ha, 1.5, 0.12)
            else:
                hmm.set_expression(rows, expr_threshold=1.5, sigma=0.12)
            first = False
            hmm.run()
            hmm.grid()                                   # warm: dosages on the device, as after the command's grid pass
            for _ in range(2):
                got = hmm.match()
            pass_ms = hmm.match_info()["last_ms"]
            after_grid = best_of(a.runs, hmm.match)

            def alone():
                hmm.grid(sample=0)                       # the handle's dosages are another call's now: not timed
                t = time.perf_counter()
                hmm.match()
                return time.perf_counter() - t
            wall_alone = min(alone() for _ in range(a.runs)) * 1e3
            flops = 2.0 * n * M * K
            nbytes = 8.0 * ((n + M) * K + n * len(chroms) * (M + 1))
            floor_ms = max(nbytes / HBM_BYTES_PER_S, flops / F64_MFMA_FLOPS) * 1e3
            entry = dict(pass_ms=round(pass_ms, 4), wall_after_grid_ms=round(after_grid, 4), wall_alone_ms=round(wall_alone, 4),
                         grid_pass_ms=round(hmm.grid_info()[1], 4), flops=flops, tflops=round(flops / pass_ms / 1e9, 3),
                         bytes=nbytes, gb_per_s=round(nbytes / pass_ms / 1e6, 1),
                         hbm_floor_ms=round(nbytes / HBM_BYTES_PER_S * 1e3, 4), mfma_floor_ms=round(flops / F64_MFMA_FLOPS * 1e3, 4),
                         bound="matrix pipe" if flops / F64_MFMA_FLOPS > nbytes / HBM_BYTES_PER_S else "HBM",
                         share_of_floor=round(floor_ms / pass_ms, 4), panel_upload_s=round(upload_s, 3))
            if (M, n) in host_at:
                if by_chrom is None:                     # the panel as the host route wants it, made outside the timing
                    by_chrom = [np.ascontiguousarray(np.stack([e[o:o + m].reshape(-1) for e in entries[:M]]))
                                for o, m in zip(offsets, points)]
                kept = {}

                def host():
                    d = hmm.grid()["dosage"]
                    kept["cross"] = [d[:, o:o + m].reshape(n, -1) @ b.T for (o, m), b in zip(zip(offsets, points), by_chrom)]
                host_ms = best_of(a.runs, host)
                worst = max(float(np.max(np.abs(got["cross"][:, c] - x) / x)) for c, x in enumerate(kept["cross"]))
                result["host_route"][f"{M}x{n}"] = dict(host_ms=round(host_ms, 3), device_wall_alone_ms=entry["wall_alone_ms"],
                                                        device_wall_after_grid_ms=entry["wall_after_grid_ms"],
                                                        max_relative_difference=worst,
                                                        met=bool(entry["wall_alone_ms"] < host_ms))
            result["passes"][f"{M}x{n}"] = entry
            print(f"{M} entries x {n} samples: {entry}", flush=True)
    result["device_bytes"] = hmm.match_info()["device_bytes"]
    hmm.close()
    line = json.dumps(result)
    print(line)
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(line + "\n")
    failed = [k for k, v in result["host_route"].items() if not v["met"]]
    if failed:
        sys.exit(f"the match pass took longer than the host route at {failed}")


if __name__ == "__main__":
    main()
