"""get-common-alignments / combine / pull-out-unique-reads / stencil / count-alignments without a device: the numpy
restatement against what the reference produced (tests/golden/matops_*.npz, scripts/gen_golden_matops.py), the
command line, and the checks gbrs_amd/matops.py makes before its first device call."""
import inspect
import os

import numpy as np
import pytest

import matops_restate as rs
from conftest import golden_files, load_golden

MATRICES = ("common", "combined", "stencil", "uniq_plain_allele", "uniq_plain_locus", "uniq_group_allele",
            "uniq_group_locus")
KEEPS = ("keep_plain_allele", "keep_plain_locus", "keep_group_allele", "keep_group_locus")


def golden_matrix(g, key):
    """(indptr list, indices list) of one matrix of a matops_*.npz fixture, as uint32."""
    ip = g[f"{key}_indptr"].astype(np.uint32)
    cuts = np.concatenate(([0], np.cumsum(ip[:, -1].astype(np.int64))))
    ix = g[f"{key}_indices"].astype(np.uint32)
    return [np.ascontiguousarray(p) for p in ip], [np.ascontiguousarray(ix[cuts[h]:cuts[h + 1]]) for h in range(len(ip))]


def golden_case(g):
    R, H, L = int(g["num_rows"]), int(g["num_haps"]), int(g["num_loci"])
    gp, gm = g["group_ptr"], g["group_members"]
    return dict(R=R, H=H, L=L, a=golden_matrix(g, "a"), b=golden_matrix(g, "b"), locus_group=g["locus_group"],
                allowed=g["allowed"], calls=[tuple(int(x) for x in c) for c in g["calls"]],
                groups=[[int(x) for x in gm[gp[i]:gp[i + 1]]] for i in range(len(gp) - 1)])


def assert_same(got, want):
    assert len(got[0]) == len(want[0])
    for h in range(len(want[0])):
        np.testing.assert_array_equal(got[0][h], want[0][h])
        np.testing.assert_array_equal(got[1][h], want[1][h])


def write_case_files(tmp_path, c, ext=".npz", count=False, names=True):
    """a and b as EMASE files plus the group and genotype files of the case."""
    from gbrs_amd.alignment import AlignmentPropertyMatrix
    R, H, L = c["R"], c["H"], c["L"]
    hname = [chr(65 + h) for h in range(H)]
    lname = [f"T{l:05d}" for l in range(L)]
    rname = np.array([f"read{k:06d}".encode() for k in range(R)]) if names else None
    paths = {}
    for tag in "ab":
        cnt = (np.arange(R) % 5 + 1).astype(np.float64) if count else None
        apm = AlignmentPropertyMatrix(shape=(L, H, R), indptr=c[tag][0], indices=c[tag][1], count=cnt,
                                      haplotype_names=hname, locus_names=lname, read_names=rname)
        paths[tag] = str(tmp_path / f"{tag}{ext}")
        apm.save(paths[tag])
    paths["groups"] = str(tmp_path / "groups.tsv")
    with open(paths["groups"], "w") as fh:
        for g, members in enumerate(c["groups"]):
            fh.write(f"G{g:05d}\t" + "\t".join(lname[l] for l in members) + "\n")
    paths["genotypes"] = str(tmp_path / "genotypes.tsv")
    with open(paths["genotypes"], "w") as fh:
        fh.write("#Gene_ID\tDiplotype\n")
        for g, (x, y) in enumerate(c["calls"]):
            fh.write(f"G{g:05d}\t{hname[x]}{hname[y]}\n")
    return paths


@pytest.mark.parametrize("path", golden_files("matops"), ids=lambda p: p.split("/")[-1][:-4])
def test_restatement_matches_reference(path):
    g = load_golden(path)
    c = golden_case(g)
    got = rs.restate_all(c)
    rs.check_not_vacuous(c, got)
    for key in MATRICES:
        assert_same(got[key], golden_matrix(g, key))
    for key in KEEPS:
        np.testing.assert_array_equal(got[key], np.unpackbits(g[key])[:c["R"]].astype(bool))
    # canonical() puts shuffled columns back in the order every result has
    rng = np.random.default_rng(0)
    shuffled = [np.concatenate([rng.permutation(ix[p[l]:p[l + 1]]) for l in range(c["L"])]).astype(np.uint32)
                if len(ix) else ix for p, ix in zip(*c["a"])]
    assert any(not np.array_equal(s, i) for s, i in zip(shuffled, c["a"][1]))
    assert_same(rs.canonical(c["R"], c["L"], c["H"], c["a"][0], shuffled), c["a"])


def test_fixture_recipe_is_not_vacuous():
    """The recipe at the size the generator's conditions were first checked at."""
    c = rs.make_case(5000, 8, 300, 1)
    out = rs.restate_all(c)
    rs.check_not_vacuous(c, out)
    for m in out.values():
        if isinstance(m, tuple):
            for p, ix in zip(*m):
                for l in np.flatnonzero(np.diff(p.astype(np.int64)) > 1):
                    assert (np.diff(ix[p[l]:p[l + 1]].astype(np.int64)) > 0).all()


def test_known_answers_by_hand():
    # H=1, L=3, R=4.  a: l0 {0,1,2}, l1 {1}, l2 {3};  b: l0 {1,2,3}, l1 {}, l2 {3}
    a = ([np.array([0, 3, 4, 5], dtype=np.uint32)], [np.array([0, 1, 2, 1, 3], dtype=np.uint32)])
    b = ([np.array([0, 3, 3, 4], dtype=np.uint32)], [np.array([1, 2, 3, 3], dtype=np.uint32)])
    ip, ix = rs.intersect(4, 3, 1, a, b)
    assert ip[0].tolist() == [0, 2, 2, 3] and ix[0].tolist() == [1, 2, 3]
    ip, ix = rs.append_rows(4, 4, 3, 1, a, b)
    assert ip[0].tolist() == [0, 6, 7, 9] and ix[0].tolist() == [0, 1, 2, 5, 6, 7, 1, 3, 7]
    assert rs.unique_rows(4, 3, 1, a[0], a[1]).tolist() == [True, False, True, True]
    # l0 and l1 one gene, l2 in none: read 1 is unique at the gene level, read 3 has no counted entry
    grp = np.array([0, 0, -1])
    assert rs.unique_rows(4, 3, 1, a[0], a[1], grp, True).tolist() == [True, True, True, False]
    ip, ix = rs.keep_rows(4, 3, 1, a[0], a[1], np.array([True, True, False, False]))
    assert ip[0].tolist() == [0, 2, 3, 3] and ix[0].tolist() == [0, 1, 1]
    ip, ix = rs.mask_columns(4, 3, 1, a[0], a[1], np.array([1, 0, 1]))
    assert ip[0].tolist() == [0, 3, 3, 4] and ix[0].tolist() == [0, 1, 2, 3]


def test_argument_parser(tmp_path):
    from gbrs_amd.cli import build_parser
    f = tmp_path / "a.npz"
    f.write_bytes(b"x")
    f, real = str(f), os.path.realpath(str(f))
    ap = build_parser()
    a = ap.parse_args(["get-common-alignments", "-i", "x.h5,y.h5", "-i", "z.h5"])
    assert (a.emase_files, a.output_file, a.comp_lib, a.verbose, a.device) == (["x.h5,y.h5", "z.h5"], None, "zlib", 0, 0)
    a = ap.parse_args(["get-common-alignments", "--emase-file", "x.h5", "--output", "o.h5", "--comp-lib", "lzo", "-vv",
                       "--device", "2"])
    assert (a.emase_files, a.output_file, a.comp_lib, a.verbose, a.device) == (["x.h5"], "o.h5", "lzo", 2, 2)
    a = ap.parse_args(["combine", "-i", "x.h5", "-i", "y.h5", "-o", "o.h5"])
    assert (a.emase_files, a.output_file, a.comp_lib, a.verbose, a.device) == (["x.h5", "y.h5"], "o.h5", "zlib", 0, 0)
    with pytest.raises(SystemExit):
        ap.parse_args(["combine", "-i", "x.h5"])                           # -o is required
    a = ap.parse_args(["pull-out-unique-reads", "-i", f, "-o", "u.h5"])
    assert (a.alignment_file, a.output_file, a.group_file, a.shallow, a.ignore_alleles, a.verbose, a.device) == \
        (real, "u.h5", None, False, False, 0, 0)
    a = ap.parse_args(["pull-out-unique-reads", "--alignment-file", f, "--output", "u.h5", "--group-file", f,
                       "--shallow", "--ignore-alleles", "-v"])
    assert (a.group_file, a.shallow, a.ignore_alleles, a.verbose) == (real, True, True, 1)
    a = ap.parse_args(["pull-out-unique-reads", "-i", f, "-o", "u.h5", "-g", f, "-s", "-a"])
    assert (a.group_file, a.shallow, a.ignore_alleles) == (real, True, True)
    with pytest.raises(SystemExit):
        ap.parse_args(["pull-out-unique-reads", "-i", f])
    a = ap.parse_args(["count-alignments", "-i", f, "-g", f])
    assert (a.alignment_file, a.group_file, a.outbase, a.verbose, a.device) == (real, real, "emase", 0, 0)
    assert ap.parse_args(["count-alignments", "-i", f, "-g", f, "--outbase", "x"]).outbase == "x"
    with pytest.raises(SystemExit):
        ap.parse_args(["count-alignments", "-i", f])                       # -g is required
    a = ap.parse_args(["stencil", "-i", f, "-G", f])
    assert (a.alignment_file, a.genotype_file, a.group_file, a.output_file, a.verbose, a.device) == \
        (real, real, None, None, 0, 0)
    a = ap.parse_args(["stencil", "--alignment-file", f, "--genotype", f, "--group-file", f, "--output", "s.h5"])
    assert (a.group_file, a.output_file) == (real, "s.h5")
    with pytest.raises(SystemExit):
        ap.parse_args(["stencil", "-i", f])                                # -G is required
    with pytest.raises(SystemExit):
        ap.parse_args(["stencil", "-i", str(tmp_path / "missing.h5"), "-G", f])


def test_function_defaults():
    from gbrs_amd import matops
    want = {
        "get_common_alignments": dict(emase_files=inspect.Parameter.empty, output_file=None, comp_lib="zlib", device=0),
        "combine": dict(emase_files=inspect.Parameter.empty, output_file=inspect.Parameter.empty, comp_lib="zlib", device=0),
        "pull_out_unique_reads": dict(alignment_file=inspect.Parameter.empty, output_file=inspect.Parameter.empty,
                                      group_file=None, shallow=False, ignore_alleles=False, device=0),
        "stencil": dict(alignment_file=inspect.Parameter.empty, genotype_file=inspect.Parameter.empty, group_file=None,
                        output_file=None, device=0),
        "count_alignments": dict(alignment_file=inspect.Parameter.empty, group_file=inspect.Parameter.empty,
                                 outbase="emase", device=0),
    }
    for name, params in want.items():
        p = inspect.signature(getattr(matops, name)).parameters
        assert list(p)[:len(params)] == list(params), name
        assert {k: p[k].default for k in params} == params, name


class _NoDevice:
    """MatOps stand-in: reaching the device in a test of the pre-device checks is a failure; in the tests of the
    default output names it marks the point the command got to."""

    def __init__(self, *a, **kw):
        raise AssertionError("device reached")


@pytest.fixture
def case_files(tmp_path, monkeypatch):
    from gbrs_amd import matops
    monkeypatch.setattr(matops, "MatOps", _NoDevice)
    monkeypatch.setattr(matops._lib, "warm_up_device_async", lambda device=0: None)
    monkeypatch.chdir(tmp_path)
    monkeypatch.setenv("GBRS_DATA", str(tmp_path / "nowhere"))
    c = golden_case(load_golden(golden_files("matops")[0]))
    return c, write_case_files(tmp_path, c), tmp_path


def test_read_names_must_agree(case_files, caplog):
    from gbrs_amd import matops
    from gbrs_amd.alignment import AlignmentPropertyMatrix
    c, paths, tmp = case_files
    R, H, L = c["R"], c["H"], c["L"]
    other = np.array([f"read{k:06d}".encode() for k in range(R)])
    other[3] = b"someoneelse"
    for tag, names in (("renamed", other), ("nameless", None)):
        AlignmentPropertyMatrix(shape=(L, H, R), indptr=c["b"][0], indices=c["b"][1], read_names=names).save(
            str(tmp / f"{tag}.npz"))
        with caplog.at_level("ERROR", logger="gbrs"):
            caplog.clear()
            with pytest.raises(ValueError, match="The read ID's are not compatible."):
                matops.get_common_alignments([paths["a"], str(tmp / f"{tag}.npz")], str(tmp / "o.npz"))
            assert "The read ID's are not compatible." in caplog.text
    # equal names, and no names at all, pass the check and go on to the device
    with pytest.raises(AssertionError, match="device reached"):
        matops.get_common_alignments([paths["a"], paths["b"]], str(tmp / "o.npz"))
    with pytest.raises(AssertionError, match="device reached"):
        matops.get_common_alignments([str(tmp / "nameless.npz"), str(tmp / "nameless.npz")], str(tmp / "o.npz"))


def test_shapes_must_agree(case_files):
    from gbrs_amd import matops
    from gbrs_amd.alignment import AlignmentPropertyMatrix
    c, paths, tmp = case_files
    R, H, L = c["R"], c["H"], c["L"]
    names = np.array([f"read{k:06d}".encode() for k in range(R + 1)])
    ip = [np.zeros(L + 1, dtype=np.uint32) for _ in range(H)]
    ix = [np.zeros(0, dtype=np.uint32) for _ in range(H)]
    AlignmentPropertyMatrix(shape=(L, H, R + 1), indptr=ip, indices=ix, read_names=names).save(str(tmp / "longer.npz"))
    AlignmentPropertyMatrix(shape=(L + 1, H, R), indptr=[np.zeros(L + 2, dtype=np.uint32)] * H, indices=ix,
                            read_names=names[:R]).save(str(tmp / "wider.npz"))
    with pytest.raises(RuntimeError, match="do not share"):
        matops.get_common_alignments([paths["a"], str(tmp / "longer.npz")], str(tmp / "o.npz"))
    with pytest.raises(RuntimeError, match="do not share"):
        matops.get_common_alignments([paths["a"], str(tmp / "wider.npz")], str(tmp / "o.npz"))
    with pytest.raises(RuntimeError, match="do not share"):
        matops.combine([paths["a"], str(tmp / "wider.npz")], str(tmp / "o.npz"))
    with pytest.raises(AssertionError, match="device reached"):             # another number of reads is what combine is for
        matops.combine([paths["a"], str(tmp / "longer.npz")], str(tmp / "o.npz"))


def test_stored_values_are_refused(case_files):
    from gbrs_amd import matops
    from gbrs_amd.alignment import AlignmentPropertyMatrix
    c, paths, tmp = case_files
    R, H, L = c["R"], c["H"], c["L"]
    AlignmentPropertyMatrix(shape=(L, H, R), indptr=c["a"][0], indices=c["a"][1],
                            values=[np.full(len(i), 0.5) for i in c["a"][1]], haplotype_names=[chr(65 + h) for h in range(H)],
                            locus_names=[f"T{l:05d}" for l in range(L)]).save(str(tmp / "valued.npz"))
    with pytest.raises(RuntimeError, match="stored values"):
        matops.pull_out_unique_reads(str(tmp / "valued.npz"), str(tmp / "o.npz"))
    with pytest.raises(RuntimeError, match="stored values"):
        matops.stencil(str(tmp / "valued.npz"), paths["genotypes"], paths["groups"], str(tmp / "o.npz"))
    with pytest.raises(AssertionError, match="device reached"):             # presence is all the intersection looks at
        matops.get_common_alignments([str(tmp / "valued.npz"), str(tmp / "valued.npz")], str(tmp / "o.npz"))


def test_a_locus_in_two_groups_is_refused(case_files):
    from gbrs_amd import matops
    c, paths, tmp = case_files
    twice = str(tmp / "twice.tsv")
    with open(paths["groups"]) as fh, open(twice, "w") as out:
        out.write(fh.read() + "GEXTRA\tT00000\n")
    with pytest.raises(RuntimeError, match="more than one group"):
        matops.pull_out_unique_reads(paths["a"], str(tmp / "o.npz"), group_file=twice)
    with pytest.raises(RuntimeError, match="more than one group"):
        matops.count_alignments(paths["a"], twice, outbase=str(tmp / "cnt"))


def test_default_output_names(case_files, caplog):
    from gbrs_amd import matops
    c, paths, tmp = case_files
    with caplog.at_level(19, logger="gbrs"):
        with pytest.raises(AssertionError, match="device reached"):
            matops.get_common_alignments([paths["a"], paths["b"]])
        assert "Output File: alignments.common.a.npz" in caplog.text
        assert f"Loading EMASE file: {paths['a']}" in caplog.text and f"Loading EMASE file: {paths['b']}" in caplog.text
        caplog.clear()
        with pytest.raises(AssertionError, match="device reached"):
            matops.stencil(paths["a"], paths["genotypes"], paths["groups"])
        assert "Output File: gbrs.stenciled.a.npz" in caplog.text
        caplog.clear()
        # no group file anywhere: the genotype file's first column would have to name loci, and this one names genes
        with pytest.raises(KeyError):
            matops.stencil(paths["a"], paths["genotypes"])
        assert "A group file is *not* given. Genotype will be stenciled as is." in caplog.text


def test_commands_log_errors_and_return_zero(case_files, caplog):
    from gbrs_amd import cli
    c, paths, tmp = case_files
    with caplog.at_level("ERROR", logger="gbrs"):
        assert cli.main(["combine", "-i", paths["a"] + "," + str(tmp / "missing.npz"), "-o", str(tmp / "o.npz")]) == 0
        assert "does not exist" in caplog.text
        assert cli.main(["get-common-alignments", "-i", paths["a"], "-i", paths["b"], "-o", str(tmp / "o.npz")]) == 0
        assert "device reached" in caplog.text
    assert not os.path.exists(tmp / "o.npz")


def test_no_cpu_fallback(hip_lib):
    import ctypes as C
    from gbrs_amd import _lib
    if hip_lib.gbrs_device_count() > 0:
        pytest.skip("a HIP device is visible")
    ip = [np.zeros(3, dtype=np.uint32)]
    ix = [np.zeros(0, dtype=np.uint32)]
    h = C.c_void_p()
    assert hip_lib.gbrs_matops_create(1, 2, 1, _lib.ptr_table(ip), _lib.ptr_table(ix), 0, C.byref(h)) == \
        _lib.GBRS_ERR_NO_DEVICE
    # arguments are checked before the device is looked for
    assert hip_lib.gbrs_matops_create(1 << 32, 2, 1, _lib.ptr_table(ip), _lib.ptr_table(ix), 0, C.byref(h)) == \
        _lib.GBRS_ERR_UNSUPPORTED
    bad = [np.array([0, 2, 1], dtype=np.uint32)]
    assert hip_lib.gbrs_matops_create(4, 2, 1, _lib.ptr_table(bad), _lib.ptr_table(ix), 0, C.byref(h)) == \
        _lib.GBRS_ERR_INVALID
