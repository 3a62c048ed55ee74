"""get-common-alignments / combine / pull-out-unique-reads / stencil on the device (gbrs_matops_*, needs an MI355X):
exact against the reference's results (tests/golden/matops_*.npz) and against the numpy restatement."""
import json
import os

import numpy as np
import pytest

import matops_restate as rs
from conftest import golden_files, load_golden
from test_matops_cpu import KEEPS, MATRICES, assert_same, golden_case, golden_matrix, write_case_files

pytestmark = pytest.mark.gpu


def apm_of(c, m, R=None, count=None):
    from gbrs_amd.alignment import AlignmentPropertyMatrix
    return AlignmentPropertyMatrix(shape=(c["L"], c["H"], c["R"] if R is None else R), indptr=m[0], indices=m[1],
                                   count=count)


def shuffled_columns(m, seed):
    """The same matrix with the row ids of every column in random order (the general route sorts them back)."""
    rng = np.random.default_rng(seed)
    out = []
    for p, ix in zip(*m):
        p = p.astype(np.int64)
        out.append(np.concatenate([rng.permutation(ix[p[l]:p[l + 1]]) for l in range(len(p) - 1)] +
                                  [np.zeros(0, dtype=np.uint32)]).astype(np.uint32))
    assert any(not np.array_equal(a, b) for a, b in zip(out, m[1]))
    return m[0], out


def device_all(c, a=None, b=None):
    """Every operation of restate_all on the device; also returns how many haplotype arrays needed the radix sort."""
    from gbrs_amd.matops import MatOps
    a, b = a or c["a"], b or c["b"]
    out, sorts = {}, 0

    def run(key, edit):
        nonlocal sorts
        with MatOps(apm_of(c, a)) as dev:
            extra = edit(dev)
            R, ip, ix = dev.get()
            sorts += dev.sizes()[2]
        out[key] = (ip, ix)
        return R, extra
    run("common", lambda d: d.intersect(apm_of(c, b)))
    R, _ = run("combined", lambda d: d.append_rows(apm_of(c, b)))
    assert R == 2 * c["R"]
    run("stencil", lambda d: d.mask_columns(c["allowed"]))
    G = len(c["groups"])
    for tag, grp in (("plain", None), ("group", c["locus_group"])):
        for lvl, ign in (("allele", False), ("locus", True)):
            _, keep = run(f"uniq_{tag}_{lvl}", lambda d: d.keep_unique_rows(grp, G if grp is not None else 0, ign))
            out[f"keep_{tag}_{lvl}"] = keep
    return out, sorts


@pytest.mark.parametrize("path", golden_files("matops"), ids=lambda p: p.split("/")[-1][:-4])
def test_device_matches_reference_golden(path):
    g = load_golden(path)
    c = golden_case(g)
    assert golden_files("matops")
    got, sorts = device_all(c)
    assert sorts == 0                                   # the fixtures' columns ascend: the sorted route
    rs.check_not_vacuous(c, got)
    for key in MATRICES:
        assert_same(got[key], golden_matrix(g, key))
    for key in KEEPS:
        np.testing.assert_array_equal(got[key], np.unpackbits(g[key])[:c["R"]].astype(bool))
    # the general route: shuffled columns, identical output
    got2, sorts2 = device_all(c, a=shuffled_columns(c["a"], 1), b=shuffled_columns(c["b"], 2))
    assert sorts2 > 0
    for key in MATRICES:
        assert_same(got2[key], golden_matrix(g, key))


@pytest.mark.parametrize("R,H,L,seed", [(5000, 8, 300, 1), (20000, 2, 500, 2), (3000, 16, 120, 3), (60000, 8, 2000, 4)])
def test_device_matches_restatement(R, H, L, seed):
    from gbrs_amd.matops import MatOps
    c = rs.make_case(R, H, L, seed)
    want = rs.restate_all(c)
    rs.check_not_vacuous(c, want)
    assert any((np.diff(p.astype(np.int64)) == 0).any() for p in c["a"][0])         # empty columns are part of it
    got, sorts = device_all(c)
    assert sorts == 0
    for key in MATRICES:
        assert_same(got[key], want[key])
    for key in KEEPS:
        np.testing.assert_array_equal(got[key], want[key])
    got2, sorts2 = device_all(c, a=shuffled_columns(c["a"], seed), b=shuffled_columns(c["b"], seed + 1))
    assert sorts2 > 0
    for key in MATRICES:
        assert_same(got2[key], want[key])
    # three operands: a third file made from b the way b was made from a
    rng = np.random.default_rng(seed + 77)
    third = rs.keep_rows(R, L, H, c["b"][0], c["b"][1], rng.random(R) < 0.7)
    with MatOps(apm_of(c, c["a"])) as dev:
        dev.intersect(apm_of(c, c["b"]))
        dev.intersect(apm_of(c, shuffled_columns(third, 5)))
        _, ip, ix = dev.get()
    w3 = rs.intersect(R, L, H, want["common"], third)
    assert 0 < sum(rs.nnz(w3)) < sum(rs.nnz(want["common"]))
    assert_same((ip, ix), w3)
    with MatOps(apm_of(c, c["a"])) as dev:
        dev.append_rows(apm_of(c, c["b"]))
        dev.append_rows(apm_of(c, third))
        R3, ip, ix = dev.get()
    assert R3 == 3 * R
    assert_same((ip, ix), rs.append_rows(2 * R, R, L, H, want["combined"], third))
    # an empty result, and edits of an empty tensor
    empty = ([np.zeros(L + 1, dtype=np.uint32) for _ in range(H)], [np.zeros(0, dtype=np.uint32) for _ in range(H)])
    with MatOps(apm_of(c, c["a"])) as dev:
        dev.intersect(apm_of(c, empty))
        assert dev.sizes()[1].sum() == 0
        assert not dev.keep_unique_rows().any()
        dev.mask_columns(c["allowed"])
        dev.append_rows(apm_of(c, c["b"]))
        R2, ip, ix = dev.get()
    assert R2 == 2 * R
    assert_same((ip, ix), rs.append_rows(R, R, L, H, empty, c["b"]))


def test_bad_operands_are_refused():
    from gbrs_amd import _lib
    from gbrs_amd.matops import MatOps
    c = rs.make_case(500, 2, 30, 9)
    bad = (c["b"][0], [i.copy() for i in c["b"][1]])
    bad[1][1][7] = 500                                  # row id == R
    with pytest.raises(_lib.GbrsHipError) as e:
        MatOps(apm_of(c, bad))
    assert e.value.status == _lib.GBRS_ERR_INVALID
    with MatOps(apm_of(c, c["a"])) as dev:
        with pytest.raises(_lib.GbrsHipError) as e:
            dev.intersect(apm_of(c, bad))
        assert e.value.status == _lib.GBRS_ERR_INVALID
    with MatOps(apm_of(c, c["a"])) as dev:
        with pytest.raises(_lib.GbrsHipError) as e:
            dev.mask_columns(np.full(30, 4, dtype=np.uint32))          # haplotype 2 of 2
        assert e.value.status == _lib.GBRS_ERR_INVALID
        with pytest.raises(_lib.GbrsHipError) as e:
            dev.keep_unique_rows(np.full(30, 3, dtype=np.int32), 3)      # group 3 of 3
        assert e.value.status == _lib.GBRS_ERR_INVALID
        with pytest.raises(RuntimeError, match="do not share"):
            wider = rs.make_case(500, 2, 31, 9)
            dev.append_rows(apm_of(wider, wider["b"]))


def _formats():
    exts = [".npz"]
    try:
        from gbrs_amd import emase_h5
        emase_h5._load()
        exts.append(".h5")
    except ImportError:
        pass
    return exts


def _load(path):
    from gbrs_amd.alignment import load_alignment, read_rname
    return load_alignment(path), read_rname(path)


@pytest.mark.parametrize("ext", _formats())             # .h5 where libhdf5 loads
@pytest.mark.parametrize("count", [False, True], ids=["plain", "count"])
def test_commands_file_to_file(tmp_path, ext, count):
    from gbrs_amd import cli
    c = golden_case(load_golden(golden_files("matops")[0]))
    want = rs.restate_all(c)
    R, H, L = c["R"], c["H"], c["L"]
    p = write_case_files(tmp_path, c, ext=ext, count=count)
    names = np.array([f"read{k:06d}".encode() for k in range(R)])
    cnt = (np.arange(R) % 5 + 1).astype(np.float64)
    out = str(tmp_path / ("out" + ext))

    assert cli.main(["get-common-alignments", "-i", p["a"] + "," + p["b"], "-o", out]) == 0
    m, rn = _load(out)
    assert m.shape == (L, H, R) and m.count is None and m.values is None
    assert_same((m.indptr, m.indices), want["common"])
    np.testing.assert_array_equal(rn, names)
    assert m.hname == [chr(65 + h) for h in range(H)] and m.lname == [f"T{l:05d}" for l in range(L)]
    os.remove(out)

    assert cli.main(["combine", "-i", p["a"], "-i", p["b"], "-o", out]) == 0
    m, rn = _load(out)
    assert m.shape == (L, H, 2 * R)
    assert_same((m.indptr, m.indices), want["combined"])
    np.testing.assert_array_equal(rn, np.concatenate((names, names)))
    if count:
        np.testing.assert_array_equal(m.count, np.concatenate((cnt, cnt)))
    else:
        assert m.count is None
    os.remove(out)

    for tag, grp in (("plain", []), ("group", ["-g", p["groups"]])):
        for lvl, flag in (("allele", []), ("locus", ["-a"])):
            assert cli.main(["pull-out-unique-reads", "-i", p["a"], "-o", out] + grp + flag) == 0
            m, rn = _load(out)
            assert m.shape == (L, H, R)
            assert_same((m.indptr, m.indices), want[f"uniq_{tag}_{lvl}"])
            np.testing.assert_array_equal(rn, names)
            if count:
                np.testing.assert_array_equal(m.count, np.where(want[f"keep_{tag}_{lvl}"], cnt, 0.0))
            os.remove(out)
    assert cli.main(["pull-out-unique-reads", "-i", p["a"], "-o", out, "-s"]) == 0
    m, rn = _load(out)
    assert rn is None and m.lname is None and m.hname is None
    assert_same((m.indptr, m.indices), want["uniq_plain_allele"])
    os.remove(out)

    assert cli.main(["stencil", "-i", p["a"], "-G", p["genotypes"], "-g", p["groups"], "-o", out]) == 0
    m, rn = _load(out)
    assert_same((m.indptr, m.indices), want["stencil"])
    np.testing.assert_array_equal(rn, names)
    if count:
        np.testing.assert_array_equal(m.count, cnt)
    os.remove(out)

    # count-alignments = the two reports `quantify -a` writes
    from gbrs_amd.alignment import load_alignment
    from gbrs_amd.counts import report_alignment_counts
    base = str(tmp_path / "cnt")
    assert cli.main(["count-alignments", "-i", p["a"], "-g", p["groups"], "-o", base]) == 0
    apm = load_alignment(p["a"], grpfile=p["groups"])
    for level, grp_wise in (("isoforms", False), ("genes", True)):
        ref = str(tmp_path / f"ref.{level}")
        report_alignment_counts(apm, ref, grp_wise=grp_wise)
        assert open(f"{base}.{level}.alignment_counts").read() == open(ref).read()


def test_launchers_accept_the_commands(tmp_path):
    import subprocess
    import sys
    from conftest import ROOT
    c = golden_case(load_golden(golden_files("matops")[0]))
    p = write_case_files(tmp_path, c)
    want = rs.restate_all(c)
    for prog in ("gbrs", "emase"):
        out = str(tmp_path / f"{prog}.npz")
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bin", prog), "get-common-alignments", "-i", p["a"], "-i",
                            p["b"], "-o", out], cwd=str(tmp_path), capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        m, _ = _load(out)
        assert_same((m.indptr, m.indices), want["common"])


def _support_files(tmp_path, c):
    lens = str(tmp_path / "lengths.info")
    rng = np.random.default_rng(3)
    with open(lens, "w") as fh:
        for l in range(c["L"]):
            n = int(rng.integers(300, 3000))
            for h in range(c["H"]):
                fh.write(f"T{l:05d}_{chr(65 + h)}\t{n}\n")
    return lens


def _table(path, H):
    rows = [line.rstrip("\n").split("\t") for line in open(path)]
    return [r[0] for r in rows[1:]], np.array([[float(x) for x in r[1:H + 2]] for r in rows[1:]])


REPORTS = [f"{level}.{what}" for level in ("isoforms", "genes") for what in ("tpm", "expected_read_counts")]


def test_common_alignments_feed_compress_and_quantify(tmp_path, monkeypatch):
    """get-common-alignments of two files -> compress -> quantify leaves the report text that compress -> quantify of
    the restated intersection leaves, character for character.

    Two `quantify` runs on one and the same file differ in the last digits of the reports, because the default E-step
    adds its partial sums through LDS float atomics in arrival order (include/gbrs_hip.h, GBRS_EM_DETERMINISTIC; measured
    here: 0.22557147114618992 against 0.22557147114618994 with array-identical compressed inputs).  That is a property
    of the EM, not of the commands under test, so both runs go through the command with the EM handle in its
    bit-reproducible mode; the comparison stays the identity of the text."""
    import functools
    from gbrs_amd import cli, quantify as quantify_module
    from gbrs_amd.alignment import AlignmentPropertyMatrix, load_alignment
    monkeypatch.setattr(quantify_module, "EMfactory", functools.partial(quantify_module.EMfactory, deterministic=True))
    monkeypatch.setenv("GBRS_DATA", str(tmp_path))
    c = rs.make_case(5000, 8, 300, 1)
    p = write_case_files(tmp_path, c)
    lens = _support_files(tmp_path, c)
    want = rs.intersect(c["R"], c["L"], c["H"], c["a"], c["b"])
    AlignmentPropertyMatrix(shape=(c["L"], c["H"], c["R"]), indptr=want[0], indices=want[1],
                            haplotype_names=[chr(65 + h) for h in range(c["H"])],
                            locus_names=[f"T{l:05d}" for l in range(c["L"])]).save(str(tmp_path / "restated.npz"))
    assert cli.main(["get-common-alignments", "-i", p["a"], "-i", p["b"], "-o", str(tmp_path / "common.npz")]) == 0
    for tag in ("common", "restated"):
        assert cli.main(["compress", "-i", str(tmp_path / f"{tag}.npz"), "-o", str(tmp_path / f"{tag}.ec.npz")]) == 0
        assert cli.main(["quantify", "-i", str(tmp_path / f"{tag}.ec.npz"), "-g", p["groups"], "-L", lens,
                         "-o", str(tmp_path / tag)]) == 0
    ea, eb = (load_alignment(str(tmp_path / f"{tag}.ec.npz")) for tag in ("common", "restated"))
    assert ea.shape == eb.shape and ea.num_reads < c["R"]
    np.testing.assert_array_equal(ea.count, eb.count)
    assert_same((ea.indptr, ea.indices), (eb.indptr, eb.indices))
    for suffix in REPORTS:
        a, b = (open(tmp_path / f"{tag}.multiway.{suffix}").read() for tag in ("common", "restated"))
        assert len(a.splitlines()) > 10
        assert a == b, suffix


def test_quantify_of_a_stenciled_file_is_quantify_with_genotypes(tmp_path, monkeypatch):
    """`quantify` of the stenciled file against `quantify -G` of the original: same iteration count, TPM and expected
    counts within the project's parity bound for those (rtol 1e-9)."""
    from gbrs_amd import cli
    monkeypatch.setenv("GBRS_DATA", str(tmp_path))
    c = rs.make_case(5000, 8, 300, 1)
    p = write_case_files(tmp_path, c)
    lens = _support_files(tmp_path, c)
    sten = str(tmp_path / "stenciled.npz")
    assert cli.main(["stencil", "-i", p["a"], "-G", p["genotypes"], "-g", p["groups"], "-o", sten]) == 0
    iters = {}
    for tag, argv in (("sten", ["-i", sten]), ("orig", ["-i", p["a"], "-G", p["genotypes"]])):
        stage = str(tmp_path / f"{tag}.stages.json")
        monkeypatch.setenv("GBRS_STAGE_TIMES", stage)
        assert cli.main(["quantify"] + argv + ["-g", p["groups"], "-L", lens, "-o", str(tmp_path / tag)]) == 0
        monkeypatch.delenv("GBRS_STAGE_TIMES")
        st = json.load(open(stage))
        assert "error" not in st, st
        iters[tag] = st["em_iterations"]
    assert iters["sten"] == iters["orig"] and iters["sten"] > 1
    for suffix in REPORTS:
        na, va = _table(tmp_path / f"sten.multiway.{suffix}", c["H"])
        nb, vb = _table(tmp_path / f"orig.diploid.{suffix}", c["H"])
        assert na == nb and va.shape == vb.shape and va.sum() > 0
        np.testing.assert_allclose(va, vb, rtol=1e-9, atol=1e-300)
