"""count-shared-multireads-pairwise without a device: the numpy restatement against what the reference produced
(tests/golden/sharedreads_*.npz, scripts/gen_golden_shared_counts.py), the command line, the checks made before the
first device call, and the writer of the count matrices."""
import inspect
import os

import numpy as np
import pytest

import shared_counts_restate as rs
from conftest import golden_files, load_golden

LEVELS = ("isoform", "gene")


def golden_case(g):
    R, H, L = int(g["num_rows"]), int(g["num_haps"]), int(g["num_loci"])
    ip = g["a_indptr"].astype(np.uint32)
    cuts = np.concatenate(([0], np.cumsum(ip[:, -1].astype(np.int64))))
    ix = g["a_indices"].astype(np.uint32)
    group = g["locus_group"].astype(np.int32)
    G = int(g["num_groups"])
    return dict(R=R, H=H, L=L, a=([np.ascontiguousarray(p) for p in ip],
                                  [np.ascontiguousarray(ix[cuts[h]:cuts[h + 1]]) for h in range(H)]),
                locus_group=group, groups=[[int(l) for l in np.flatnonzero(group == k)] for k in range(G)])


def golden_result(g, level):
    n = int(g["num_loci"] if level == "isoform" else g["num_groups"])
    return tuple(g[f"{level}_{part}"].astype(np.int64) for part in ("indptr", "indices", "data")) + (n,)


def assert_same_counts(got, want):
    assert got[3] == want[3]
    for a, b in zip(got[:3], want[:3]):
        np.testing.assert_array_equal(np.asarray(a).astype(np.int64), np.asarray(b).astype(np.int64))


def write_case_files(tmp_path, c, ext=".npz", count=False):
    """The case as an EMASE file plus its group file."""
    from gbrs_amd.alignment import AlignmentPropertyMatrix
    R, H, L = c["R"], c["H"], c["L"]
    lname = [f"T{l:05d}" for l in range(L)]
    cnt = (np.arange(R) % 5 + 1).astype(np.float64) if count else None
    paths = dict(a=str(tmp_path / f"a{ext}"), groups=str(tmp_path / "groups.tsv"))
    AlignmentPropertyMatrix(shape=(L, H, R), indptr=c["a"][0], indices=c["a"][1], count=cnt,
                            haplotype_names=[chr(65 + h) for h in range(H)], locus_names=lname).save(paths["a"])
    with open(paths["groups"], "w") as fh:
        for g, members in enumerate(c["groups"]):
            fh.write(f"G{g:05d}\t" + "\t".join(lname[l] for l in members) + "\n")
    return paths


def test_there_are_three_fixtures():
    assert [os.path.basename(p) for p in golden_files("sharedreads")] == \
        ["sharedreads_h1.npz", "sharedreads_h16.npz", "sharedreads_h8.npz"]


@pytest.mark.parametrize("path", golden_files("sharedreads"), ids=lambda p: p.split("/")[-1][:-4])
def test_restatement_matches_reference(path):
    g = load_golden(path)
    c = golden_case(g)
    got = rs.restate_both(c)
    rs.check_not_vacuous(c, got)
    for level in LEVELS:
        assert_same_counts(got[level], golden_result(g, level))
        ip, ix, data, n = got[level]
        d = rs.dense(ip, ix, data, n)
        assert (d == d.T).all() and (data > 0).all()


def test_known_answer_by_hand():
    # H=2, L=4, R=4.  read 0: loci {0, 1} (locus 0 in both haplotypes); read 1: {1, 2}; read 2: {0, 1, 3}; read 3: none
    ip = [np.array([0, 2, 3, 3, 4], dtype=np.uint32), np.array([0, 1, 3, 4, 4], dtype=np.uint32)]
    ix = [np.array([0, 2, 0, 2], dtype=np.uint32), np.array([0, 1, 2, 1], dtype=np.uint32)]
    ipc, ixc, data, n = rs.shared_counts(4, 4, 2, ip, ix)
    assert n == 4
    assert rs.dense(ipc, ixc, data, n).tolist() == [[2, 2, 0, 1], [2, 3, 1, 1], [0, 1, 1, 0], [1, 1, 0, 1]]
    assert ipc.tolist() == [0, 3, 7, 9, 12] and ixc.tolist() == [0, 1, 3, 0, 1, 2, 3, 1, 2, 0, 1, 3]
    # loci 0 and 1 one gene, locus 2 another, locus 3 in none: its entries drop out
    ipc, ixc, data, n = rs.shared_counts(4, 4, 2, ip, ix, np.array([0, 0, 1, -1]), 2)
    assert n == 2 and rs.dense(ipc, ixc, data, n).tolist() == [[3, 1], [1, 1]]


def test_generated_cases_are_not_vacuous():
    for args in ((4000, 1, 300, 21), (3000, 8, 200, 22)):
        c = rs.make_case(*args)
        rs.check_not_vacuous(c, rs.restate_both(c))
    c = rs.make_case(2000, 2, 700, 23, wide=600)
    keys, _ = rs.pattern_keys(c["R"], c["L"], c["H"], c["a"][0], c["a"][1])
    assert np.bincount(keys // c["L"]).max() == 600


def test_argument_parser(tmp_path):
    from gbrs_amd.cli import build_parser
    f = tmp_path / "a.npz"
    f.write_bytes(b"x")
    f, real = str(f), os.path.realpath(str(f))
    ap = build_parser()
    a = ap.parse_args(["count-shared-multireads-pairwise", "-i", f, "-g", f])
    assert (a.alignment_file, a.group_file, a.outbase, a.verbose, a.device, a.separate_outputs) == \
        (real, real, "emase", 0, 0, False)
    a = ap.parse_args(["count-shared-multireads-pairwise", "--alignment-file", f, "--group-file", f, "--outbase", "x",
                       "-vv", "--device", "3", "--separate-outputs"])
    assert (a.outbase, a.verbose, a.device, a.separate_outputs) == ("x", 2, 3, True)
    assert ap.parse_args(["count-shared-multireads-pairwise", "-i", f, "-g", f, "-o", "y"]).outbase == "y"
    with pytest.raises(SystemExit):
        ap.parse_args(["count-shared-multireads-pairwise", "-i", f])                      # -g is required
    with pytest.raises(SystemExit):
        ap.parse_args(["count-shared-multireads-pairwise", "-g", f])                      # -i is required
    with pytest.raises(SystemExit):
        ap.parse_args(["count-shared-multireads-pairwise", "-i", str(tmp_path / "missing.h5"), "-g", f])
    help_text = " ".join(ap._subparsers._group_actions[0].choices["count-shared-multireads-pairwise"].format_help().split())
    assert "overwrites the isoform-level one" in help_text


def test_function_defaults():
    from gbrs_amd import matops
    want = dict(alignment_file=inspect.Parameter.empty, group_file=inspect.Parameter.empty, outbase="emase", device=0,
                stage_times=None, separate_outputs=False)
    p = inspect.signature(matops.count_shared_multireads_pairwise).parameters
    assert list(p) == list(want)
    assert {k: p[k].default for k in want} == want
    p = inspect.signature(matops.MatOps.shared_counts).parameters
    assert list(p) == ["self", "locus_group", "num_groups"] and p["locus_group"].default is None and p["num_groups"].default == 0
    assert list(inspect.signature(matops.save_shared_counts).parameters) == ["path", "indptr", "indices", "data", "n"]


class _NoDevice:
    def __init__(self, *a, **kw):
        raise AssertionError("device reached")


@pytest.fixture
def case_files(tmp_path, monkeypatch):
    from gbrs_amd import matops
    monkeypatch.setattr(matops, "MatOps", _NoDevice)
    monkeypatch.setattr(matops._lib, "warm_up_device_async", lambda device=0: None)
    monkeypatch.chdir(tmp_path)
    c = golden_case(load_golden(golden_files("sharedreads")[0]))
    return c, write_case_files(tmp_path, c), tmp_path


def test_refused_before_any_device_call(case_files, monkeypatch):
    from gbrs_amd import matops
    c, paths, tmp = case_files
    with pytest.raises(RuntimeError, match="needs a group file"):
        matops.count_shared_multireads_pairwise(paths["a"], None, outbase=str(tmp / "o"))
    twice = str(tmp / "twice.tsv")
    with open(paths["groups"]) as fh, open(twice, "w") as out:
        out.write(fh.read() + "GEXTRA\tT00000\n")
    with pytest.raises(RuntimeError, match="more than one group"):
        matops.count_shared_multireads_pairwise(paths["a"], twice, outbase=str(tmp / "o"))
    with pytest.raises(AssertionError, match="device reached"):             # a good group file goes on to the device
        matops.count_shared_multireads_pairwise(paths["a"], paths["groups"], outbase=str(tmp / "o"))
    assert not [f for f in os.listdir(tmp) if "shared_read_counts" in f]

    # a map of the wrong shape: refused by MatOps.shared_counts before it touches the library
    class _NoLibrary:
        def __getattr__(self, name):
            raise AssertionError("library reached")
    monkeypatch.undo()
    dev = matops.MatOps.__new__(matops.MatOps)
    dev._lib, dev._h, dev.L, dev.H = _NoLibrary(), None, c["L"], c["H"]
    with pytest.raises(RuntimeError, match="does not match to the matrix shape"):
        dev.shared_counts(np.zeros(c["L"] + 1, dtype=np.int32), 1)
    with pytest.raises(AssertionError, match="library reached"):
        dev.shared_counts(c["locus_group"], len(c["groups"]))


def _scipy():
    try:
        import scipy.sparse
        return scipy.sparse
    except ImportError:
        return None


@pytest.mark.parametrize("path", golden_files("sharedreads"), ids=lambda p: p.split("/")[-1][:-4])
def test_writer_round_trip_plain_members(path, tmp_path, caplog):
    from gbrs_amd.matops import save_shared_counts
    g = load_golden(path)
    for level in LEVELS:
        ip, ix, data, n = golden_result(g, level)
        with caplog.at_level("WARNING", logger="gbrs"):
            caplog.clear()
            out = save_shared_counts(str(tmp_path / f"{level}.shared_read_counts"), ip, ix, data.astype(np.float64), n)
            assert ("scipy is not available" in caplog.text) == (_scipy() is None)
        assert out == str(tmp_path / f"{level}.shared_read_counts.npz") and os.path.exists(out)
        with np.load(out, allow_pickle=False) as z:
            assert {"indptr", "indices", "data", "shape"} <= set(z.files)
            np.testing.assert_array_equal(z["indptr"], ip)
            np.testing.assert_array_equal(z["indices"], ix)
            np.testing.assert_array_equal(z["data"], data)
            assert z["data"].dtype == np.float64 and z["shape"].tolist() == [n, n]
    with pytest.raises(RuntimeError, match="do not match"):
        save_shared_counts(str(tmp_path / "bad"), ip[:-1], ix, data, n)


@pytest.mark.parametrize("path", golden_files("sharedreads"), ids=lambda p: p.split("/")[-1][:-4])
def test_writer_round_trip_scipy_member(path, tmp_path):
    sparse = _scipy()
    if sparse is None:
        pytest.skip("scipy is not installed")
    from gbrs_amd.matops import save_shared_counts
    g = load_golden(path)
    for level in LEVELS:
        ip, ix, data, n = golden_result(g, level)
        out = save_shared_counts(str(tmp_path / level), ip, ix, data, n)
        with np.load(out, allow_pickle=True) as z:                # what the reference's readers do
            counts = z["counts"]
        assert counts.shape == () and counts.dtype == object
        m = counts.item()
        assert sparse.isspmatrix_csr(m) and m.dtype == np.float64 and m.shape == (n, n)
        np.testing.assert_array_equal(m.toarray(), rs.dense(ip, ix, data, n).astype(np.float64))


class _RestatedDevice:
    """MatOps stand-in that answers shared_counts with the restatement: drives the command's file handling."""

    def __init__(self, apm, device=0):
        L, H, R = apm.shape
        self.args = (R, L, H, apm.indptr, apm.indices)

    def shared_counts(self, locus_group=None, num_groups=0):
        ip, ix, data, n = rs.shared_counts(*self.args, locus_group, num_groups)
        return ip, ix.astype(np.int32), data.astype(np.float64), n

    def shared_counts_info(self):
        return dict(num_columns=0, pattern_entries=0, pairs_emitted=0, batches=0, pair_budget=0, peak_device_bytes=0,
                    device_ms=0.0)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        pass


@pytest.mark.parametrize("count", [False, True], ids=["plain", "count"])
def test_output_file_sets(tmp_path, monkeypatch, caplog, count):
    from gbrs_amd import matops
    monkeypatch.setattr(matops, "MatOps", _RestatedDevice)
    monkeypatch.setattr(matops._lib, "warm_up_device_async", lambda device=0: None)
    g = load_golden(golden_files("sharedreads")[-1])
    c = golden_case(g)
    paths = write_case_files(tmp_path, c, count=count)

    def members(path):
        with np.load(path, allow_pickle=False) as z:
            return z["indptr"], z["indices"], z["data"], int(z["shape"][0])

    def produced():
        return sorted(f for f in os.listdir(tmp_path) if "shared_read_counts" in f)
    # default: what the reference leaves - one file under the isoforms name, holding the gene-level matrix
    stages = {}
    with caplog.at_level(19, logger="gbrs"):
        matops.count_shared_multireads_pairwise(paths["a"], paths["groups"], outbase=str(tmp_path / "d"), stage_times=stages)
    assert produced() == ["d.isoforms.shared_read_counts.npz"]
    assert_same_counts(members(tmp_path / "d.isoforms.shared_read_counts.npz"), golden_result(g, "gene"))
    lines = [r.getMessage() for r in caplog.records]
    first = lines.index(f"Generating isoform Shared Read Counts: {tmp_path / 'd'}.isoforms.shared_read_counts")
    second = lines.index(f"Generating genes Shared Read Counts: {tmp_path / 'd'}.isoforms.shared_read_counts")
    assert first < second < lines.index("Done")
    assert f"Alignment File: {paths['a']}" in lines and f"Group File: {paths['groups']}" in lines
    assert f"Outbase: {tmp_path / 'd'}" in lines and f"Loading EMASE file: {paths['a']}" in lines
    assert sum("count vector" in m for m in lines) == (1 if count else 0)
    assert {"load", "upload", "kernels", "write"} <= set(stages)
    os.remove(tmp_path / "d.isoforms.shared_read_counts.npz")
    # the extension: both matrices survive
    matops.count_shared_multireads_pairwise(paths["a"], paths["groups"], outbase=str(tmp_path / "s"), separate_outputs=True)
    assert produced() == ["s.genes.shared_read_counts.npz", "s.isoforms.shared_read_counts.npz"]
    assert_same_counts(members(tmp_path / "s.isoforms.shared_read_counts.npz"), golden_result(g, "isoform"))
    assert_same_counts(members(tmp_path / "s.genes.shared_read_counts.npz"), golden_result(g, "gene"))
    assert matops.shared_counts_paths("x") == ("x.isoforms.shared_read_counts", "x.isoforms.shared_read_counts")


def test_symbols_and_null_handle(hip_lib):
    """The calls exist and check their arguments before they look for a device; there is no CPU fallback to reach."""
    from gbrs_amd import _lib
    for name in ("gbrs_matops_shared_counts", "gbrs_matops_shared_counts_get", "gbrs_matops_shared_counts_info"):
        assert name in _lib.EXPORTS and hasattr(hip_lib, name)
    assert hip_lib.gbrs_matops_shared_counts(None, None, 0, None) == _lib.GBRS_ERR_INVALID
    assert hip_lib.gbrs_matops_shared_counts_get(None, None, None, None) == _lib.GBRS_ERR_INVALID
    assert hip_lib.gbrs_matops_shared_counts_info(None, None, None, None, None, None, None, None) == _lib.GBRS_ERR_INVALID


def test_writer_without_scipy(tmp_path, monkeypatch, caplog):
    """A machine without scipy: `counts` is left out, one warning says so, the plain members are all there."""
    import sys
    from gbrs_amd.matops import save_shared_counts
    monkeypatch.setitem(sys.modules, "scipy", None)
    monkeypatch.setitem(sys.modules, "scipy.sparse", None)
    g = load_golden(golden_files("sharedreads")[0])
    ip, ix, data, n = golden_result(g, "gene")
    with caplog.at_level("WARNING", logger="gbrs"):
        out = save_shared_counts(str(tmp_path / "nos.npz"), ip, ix, data, n)
    assert sum("scipy is not available" in r.getMessage() for r in caplog.records) == 1
    with np.load(out, allow_pickle=False) as z:
        assert sorted(z.files) == ["data", "indices", "indptr", "shape"]
        assert_same_counts((z["indptr"], z["indices"], z["data"], int(z["shape"][0])), (ip, ix, data, n))
