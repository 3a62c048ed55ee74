#!/usr/bin/env python3
"""gbrs_em_resample: the blocking call's time against the cut above which a row's draws get a workgroup of their own
(GBRS_TUNING_RESAMPLE_CUT), on 2M rows x 8 x 20k with heavy-tailed counts (floor(exp(Exp(2.2))), capped at 200,000: half
the rows count at most 4, one in a hundred more than 25,000).  One child process per cut, each under a time limit; prints
one JSON line per cut (kept in profiles/resample_cut_probe.txt).  Needs an MI355X."""
import os, sys, time, json, subprocess
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if len(sys.argv) > 1:
    from gbrs_amd import synth, _lib
    from gbrs_amd.alignment import AlignmentPropertyMatrix
    from gbrs_amd.em import EMfactory
    import ctypes as C
    R = 2_000_000
    inc = synth.make_em_problem(R=R, H=8, L=20_000, seed=5)
    rng = np.random.default_rng(1)
    count = np.minimum(np.floor(np.exp(rng.exponential(2.2, R))), 2e5)
    apm = AlignmentPropertyMatrix(shape=(inc.num_loci, inc.num_haps, R), indptr=inc.indptr, indices=inc.indices, count=count,
                                  haplotype_names=inc.hap_names, locus_names=inc.locus_names)
    em = EMfactory(apm, resample=True)
    em.prepare()
    big, cut = C.c_uint64(0), C.c_uint32(0)
    _lib.load().gbrs_em_resample_info(em._h, None, C.byref(big), C.byref(cut))
    em.resample(1, 0)
    ts = []
    for b in range(1, 8):
        t = time.perf_counter(); em.resample(1, b); ts.append((time.perf_counter() - t) * 1e3)
    t = time.perf_counter(); em.resample(1, 0xFFFFFFFF); base = (time.perf_counter() - t) * 1e3
    print(json.dumps(dict(cut=cut.value, big_rows=big.value, resample_ms=round(sorted(ts)[3], 4), restore_ms=round(base, 4),
                          draws=float(count.sum()), max_count=float(count.max()), q=[float(x) for x in np.quantile(count, [.5, .9, .99, .999])])), flush=True)
    em.close()
    sys.exit(0)
for cut in (16, 64, 256, 1024, 4096, 16384, 1000000):
    r = subprocess.run(['timeout', '-k', '10', '120', sys.executable, os.path.abspath(__file__), 'child'],
                       env=dict(os.environ, GBRS_TUNING_RESAMPLE_CUT=str(cut)), stdout=subprocess.PIPE, text=True)
    if r.returncode != 0:
        print('child failed', r.returncode); sys.exit(1)
    print(r.stdout.strip().splitlines()[-1], flush=True)
