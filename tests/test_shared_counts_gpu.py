"""count-shared-multireads-pairwise on the device (gbrs_matops_shared_counts, needs an MI355X): exact against the
reference's results (tests/golden/sharedreads_*.npz) and against the numpy restatement, at both levels."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import shared_counts_restate as rs
from conftest import ROOT, golden_files, load_golden
from test_matops_gpu import shuffled_columns
from test_shared_counts_cpu import LEVELS, assert_same_counts, golden_case, golden_result, write_case_files

pytestmark = pytest.mark.gpu


def apm_of(c, m=None):
    from gbrs_amd.alignment import AlignmentPropertyMatrix
    m = m or c["a"]
    return AlignmentPropertyMatrix(shape=(c["L"], c["H"], c["R"]), indptr=m[0], indices=m[1])


def level_args(c, level):
    return (None, 0) if level == "isoform" else (c["locus_group"], len(c["groups"]))


def device_both(c, m=None):
    """{'isoform': ..., 'gene': ...} from one upload, the call's report next to each, and the tensor before / after."""
    from gbrs_amd.matops import MatOps
    out, info = {}, {}
    with MatOps(apm_of(c, m)) as dev:
        before = dev.get()
        for level in LEVELS:
            out[level] = dev.shared_counts(*level_args(c, level))
            info[level] = dev.shared_counts_info()
        after = dev.get()
        sorts = dev.sizes()[2]
    # the tensor is left untouched
    assert before[0] == after[0]
    for h in range(c["H"]):
        np.testing.assert_array_equal(before[1][h], after[1][h])
        np.testing.assert_array_equal(before[2][h], after[2][h])
    return out, info, sorts


def pairs_of(c, level):
    """The pairs (i <= j) the definition asks for: k (k + 1) / 2 per read with k distinct columns."""
    keys, n = rs.pattern_keys(c["R"], c["L"], c["H"], c["a"][0], c["a"][1], *level_args(c, level))
    k = np.bincount(keys // n, minlength=c["R"]).astype(np.int64)
    return int((k * (k + 1) // 2).sum()), len(keys), int(k.max())


def column_read_counts(c, level):
    """Reads per column from gbrs_counts_get, on the haplotypes folded into one (P itself as a 1-haplotype tensor)."""
    from gbrs_amd import _lib
    lib = _lib.load()
    R, L = c["R"], c["L"]
    keys, _ = rs.pattern_keys(R, L, c["H"], c["a"][0], c["a"][1])
    order = np.argsort((keys % L) * R + keys // L, kind="stable")
    ip = [np.searchsorted((keys % L)[order], np.arange(L + 1)).astype(np.uint32)]
    ix = [(keys // L)[order].astype(np.uint32)]
    group, G = level_args(c, level)
    n = L if group is None else G
    group = None if group is None else np.ascontiguousarray(group, dtype=np.int32)
    h = C.c_void_p()
    _lib.check(lib.gbrs_counts_create(R, L, 1, _lib.ptr_table(ip), _lib.ptr_table(ix), None, 0, C.byref(h)))
    aln, uniq, lu = np.empty((1, n)), np.empty((1, n)), np.empty(n)
    try:
        _lib.check(lib.gbrs_counts_get(h, _lib.ptr(group), n, _lib.ptr(aln), _lib.ptr(uniq), _lib.ptr(lu)))
    finally:
        lib.gbrs_counts_destroy(h)
    return aln[0]


def assert_structure(c, level, result):
    ip, ix, data, n = result
    assert ip.shape == (n + 1,) and ip[0] == 0 and ip[-1] == len(ix) == len(data) and data.dtype == np.float64
    assert (np.diff(ip) >= 0).all() and (data > 0).all() and (data == np.round(data)).all()      # no stored zeros
    rows = np.repeat(np.arange(n), np.diff(ip))
    same_row = rows[1:] == rows[:-1]
    assert (np.diff(ix.astype(np.int64))[same_row] > 0).all()                                   # ascending, no repeats
    d = rs.dense(ip, ix, data.astype(np.int64), n)
    assert (d == d.T).all()
    np.testing.assert_array_equal(np.diag(d).astype(np.float64), column_read_counts(c, level))


@pytest.mark.parametrize("path", golden_files("sharedreads"), ids=lambda p: p.split("/")[-1][:-4])
def test_device_matches_reference_golden(path):
    g = load_golden(path)
    c = golden_case(g)
    got, info, sorts = device_both(c)
    assert sorts == 0
    rs.check_not_vacuous(c, {k: (v[0], v[1], v[2].astype(np.int64), v[3]) for k, v in got.items()})
    for level in LEVELS:
        assert_same_counts(got[level], golden_result(g, level))
        assert_structure(c, level, got[level])
        pairs, entries, _ = pairs_of(c, level)
        assert (info[level]["pairs_emitted"], info[level]["pattern_entries"]) == (pairs, entries)
        assert info[level]["batches"] == 1 and info[level]["num_columns"] == got[level][3]
    # the general route: shuffled columns, identical output
    got2, _, sorts2 = device_both(c, shuffled_columns(c["a"], 1))
    assert sorts2 > 0
    for level in LEVELS:
        assert_same_counts(got2[level], golden_result(g, level))


SHAPES = [(20000, 1, 500, 31, 0), (30000, 8, 1000, 32, 0), (5000, 16, 300, 33, 0), (8000, 2, 1500, 34, 700)]


@pytest.mark.parametrize("R,H,L,seed,wide", SHAPES)
def test_device_matches_restatement(R, H, L, seed, wide, monkeypatch):
    monkeypatch.delenv("GBRS_SHARED_PAIR_BUDGET", raising=False)
    c = rs.make_case(R, H, L, seed, wide=wide)
    want = rs.restate_both(c)
    rs.check_not_vacuous(c, want)
    if wide:
        assert pairs_of(c, "isoform")[2] == wide > 500                 # a single row that hits more than 500 loci
    got, info, sorts = device_both(c)
    assert sorts == 0
    for level in LEVELS:
        assert_same_counts(got[level], want[level])
        assert_structure(c, level, got[level])
        assert info[level]["batches"] == 1 and info[level]["pairs_emitted"] == pairs_of(c, level)[0]
    # a second run gives the same arrays, and so do shuffled columns
    again, _, _ = device_both(c)
    got2, _, sorts2 = device_both(c, shuffled_columns(c["a"], seed))
    assert sorts2 > 0
    for level in LEVELS:
        for other in (again, got2):
            for a, b in zip(got[level][:3], other[level][:3]):
                np.testing.assert_array_equal(a, b)

    # the same results from many small batches, one row's pairs over the budget among them
    pairs, _, widest = pairs_of(c, "gene")
    budget = min(pairs // 9, max(1, widest * (widest + 1) // 2 - 1)) if wide else pairs // 9
    monkeypatch.setenv("GBRS_SHARED_PAIR_BUDGET", str(budget))
    small, sinfo, _ = device_both(c)
    for level in LEVELS:
        pairs, _, widest = pairs_of(c, level)
        print(f"{level}: budget {budget}, pairs {pairs}, batches {sinfo[level]['batches']}, widest row {widest}")
        assert sinfo[level]["pair_budget"] == budget
        assert sinfo[level]["batches"] == -(-pairs // budget) >= 8
        if wide:
            assert widest * (widest + 1) // 2 > budget                 # that row alone is cut into several batches
        for a, b in zip(small[level][:3], got[level][:3]):
            np.testing.assert_array_equal(a, b)


def test_budget_of_one_pair_and_an_empty_tensor(monkeypatch):
    """The extremes: every pair a batch of its own, and a tensor without entries."""
    from gbrs_amd import _lib
    from gbrs_amd.matops import MatOps
    c = rs.make_case(60, 2, 12, 5)
    want = rs.restate_both(c)
    monkeypatch.setenv("GBRS_SHARED_PAIR_BUDGET", "1")
    got, info, _ = device_both(c)
    for level in LEVELS:
        assert_same_counts(got[level], want[level])
        assert info[level]["batches"] == info[level]["pairs_emitted"] > 60
    monkeypatch.setenv("GBRS_SHARED_PAIR_BUDGET", "none")
    with MatOps(apm_of(c)) as dev:
        with pytest.raises(_lib.GbrsHipError) as e:
            dev.shared_counts()
        assert e.value.status == _lib.GBRS_ERR_INVALID
    monkeypatch.delenv("GBRS_SHARED_PAIR_BUDGET")
    empty = ([np.zeros(13, dtype=np.uint32)] * 2, [np.zeros(0, dtype=np.uint32)] * 2)
    with MatOps(apm_of(c, empty)) as dev:
        ip, ix, data, n = dev.shared_counts()
        assert n == 12 and not ip.any() and len(ix) == len(data) == 0
        assert dev.shared_counts_info()["batches"] == 0
    # every entry at loci in no group: an empty gene-level result
    none = np.full(12, -1, dtype=np.int32)
    with MatOps(apm_of(c)) as dev:
        ip, ix, data, n = dev.shared_counts(none, 3)
        assert n == 3 and not ip.any() and len(ix) == 0


def test_bad_arguments_are_refused():
    from gbrs_amd import _lib
    from gbrs_amd.matops import MatOps
    c = rs.make_case(500, 2, 30, 9)
    with MatOps(apm_of(c)) as dev:
        lib = _lib.load()
        assert lib.gbrs_matops_shared_counts_get(dev._h, None, None, None) == _lib.GBRS_ERR_INVALID
        ip = np.zeros(31, dtype=np.uint64)
        assert lib.gbrs_matops_shared_counts_get(dev._h, _lib.ptr(ip), None, None) == _lib.GBRS_ERR_INVALID   # no result yet
        with pytest.raises(_lib.GbrsHipError) as e:
            dev.shared_counts(np.full(30, 3, dtype=np.int32), 3)       # group 3 of 3
        assert e.value.status == _lib.GBRS_ERR_INVALID
        with pytest.raises(_lib.GbrsHipError) as e:
            dev.shared_counts(np.zeros(30, dtype=np.int32), 0)         # a map without groups
        assert e.value.status == _lib.GBRS_ERR_INVALID
        with pytest.raises(RuntimeError, match="does not match"):
            dev.shared_counts(np.zeros(31, dtype=np.int32), 1)
        want = rs.shared_counts(500, 30, 2, c["a"][0], c["a"][1])
        assert_same_counts(dev.shared_counts(), want)                   # the handle is still good


def _members(path):
    with np.load(path, allow_pickle=False) as z:
        return z["indptr"], z["indices"], z["data"], int(z["shape"][0])


def test_end_to_end_both_launchers(tmp_path):
    try:
        from gbrs_amd import emase_h5
        emase_h5._load()
        ext = ".h5"
    except ImportError:                                                # no libhdf5 here: the project's own format
        ext = ".npz"
    c = rs.make_case(4000, 8, 250, 41)
    want = rs.restate_both(c)
    rs.check_not_vacuous(c, want)
    p = write_case_files(tmp_path, c, ext=ext, count=True)
    for prog in ("gbrs", "emase"):
        for flags, files in (([], {"isoforms": "gene"}), (["--separate-outputs"], {"isoforms": "isoform", "genes": "gene"})):
            base = str(tmp_path / f"{prog}{len(flags)}")
            r = subprocess.run([sys.executable, os.path.join(ROOT, "bin", prog), "count-shared-multireads-pairwise", "-i",
                                p["a"], "-g", p["groups"], "-o", base, "-v"] + flags, cwd=str(tmp_path),
                               capture_output=True, text=True, timeout=300)
            assert r.returncode == 0, r.stderr
            log = r.stderr
            assert log.index("Generating isoform Shared Read Counts") < log.index("Generating genes Shared Read Counts") \
                < log.index("Done"), log
            assert "count vector" in log
            made = sorted(f for f in os.listdir(tmp_path) if f.startswith(os.path.basename(base) + "."))
            assert made == sorted(f"{os.path.basename(base)}.{name}.shared_read_counts.npz" for name in files)
            for name, level in files.items():
                assert_same_counts(_members(f"{base}.{name}.shared_read_counts.npz"), want[level])
