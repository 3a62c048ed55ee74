#!/usr/bin/env python3
"""One EM step of multiread models 1-4 on BASELINE configs[1] (40M reads x 8 haplotypes x 120k isoforms, built in HBM
by gbrs_amd.synth_torch, both variants), next to Model 4 on the CSC layout (GBRS_EM_LAYOUT_CSC) in the same process.
Also the time gbrs_em_set_groups takes (grouped layout for models 2/3), the extra time of model 1's first step (its
own order) and the device memory the grouped layout holds.  Prints one JSON line per variant.

    timeout -k 10 600 python scripts/em_models_bench.py [--steps 10]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--reads", type=int, default=40_000_000)
    args = ap.parse_args()
    import numpy as np
    import torch
    from gbrs_amd import _lib, synth, synth_torch
    lib = _lib.load()

    def create(prob, flags):
        h = C.c_void_p()
        _lib.check(lib.gbrs_em_create_device(prob["R"], prob["L"], prob["H"],
                                             _lib.raw_table([t.data_ptr() for t in prob["indptr"]]),
                                             _lib.raw_table([t.data_ptr() for t in prob["indices"]]), None,
                                             C.c_void_p(prob["eff_len"].data_ptr()), 0, flags, C.byref(h)))
        _lib.check(lib.gbrs_em_prepare(h, 0.0))
        return h

    def step_ms(h, model, n):
        _lib.check(lib.gbrs_em_step_model(h, model, 1, None))          # warm-up (and model 1's order)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _lib.check(lib.gbrs_em_step_model(h, model, n, None))
        return (time.perf_counter() - t0) * 1e3 / n

    for variant in ("survey", "multi_isoform"):
        prob = synth_torch.make_em_problem_device(args.reads, 8, 120_000, synth.SEED_BASE_EM + 1, "cuda:0",
                                                  variant=variant)
        L = prob["L"]
        starts = np.asarray(prob["gene_starts"], dtype=np.int64)
        gptr = np.concatenate((starts, [L])).astype(np.int64)
        mem = np.arange(L, dtype=np.int64)
        out = dict(variant=variant, reads=prob["R"], entries=int(prob["N"]), genes=len(starts))
        for name, flags in (("csc", _lib.GBRS_EM_LAYOUT_CSC), ("tiles", 0)):
            h = create(prob, flags)
            out[f"m4_{name}_step_ms"] = step_ms(h, 4, args.steps)
            lib.gbrs_em_destroy(h)
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        free0 = torch.cuda.mem_get_info()[0]
        h = create(prob, _lib.GBRS_EM_GROUPED_MODELS)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _lib.check(lib.gbrs_em_set_groups(h, len(starts), _lib.ptr(gptr), _lib.ptr(mem)))
        out["set_groups_ms"] = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        _lib.check(lib.gbrs_em_step_model(h, 1, 1, None))
        out["m1_first_step_ms"] = (time.perf_counter() - t0) * 1e3
        out["grouped_handle_bytes"] = int(free0 - torch.cuda.mem_get_info()[0])
        for model in (3, 2, 1, 4):
            out[f"m{model}_step_ms"] = step_ms(h, model, args.steps)
        lib.gbrs_em_destroy(h)
        out["m123_over_m4_csc"] = max(out[f"m{m}_step_ms"] for m in (1, 2, 3)) / out["m4_csc_step_ms"]
        print(json.dumps(out), flush=True)
        del prob
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
