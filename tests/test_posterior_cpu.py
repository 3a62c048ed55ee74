"""Read-level posteriors, the parts that need no GPU: the closed form against the reference's fixtures, the value
providers of the file writers, and the command-line plumbing of `--posterior-values`."""
import argparse
import os

import numpy as np
import pytest

from conftest import golden_files, load_golden
from em_models_restate import ModelsEM, fixture_inputs
from posterior_restate import masked_structure, posterior

FIXTURES = golden_files("posterior")
GOLD = os.path.dirname(FIXTURES[0]) if FIXTURES else ""


def test_fixtures_present():
    names = {os.path.basename(p)[len("posterior_"):-4] for p in FIXTURES}
    assert names == {"h8_len", "h2_count", "h16_len_count", "h1_len", "h8_mask", "h4_pseudo_values", "h8_maxiter",
                     "h8_called"}


@pytest.mark.parametrize("path", FIXTURES, ids=lambda p: os.path.basename(p)[:-4])
def test_restatement_reproduces_the_reference(path):
    """posterior_restate from m{k}_theta_before gives every m{k}_post{h} to 1e-12: the closed form is the reference's."""
    post = load_golden(path)
    g = load_golden(os.path.join(GOLD, "emmodel_m1_" + os.path.basename(path)[len("posterior_"):]))
    R, L, H, indptr, indices, count, eff_len, groups, gtmask, values = fixture_inputs(g)
    cpu = ModelsEM(R, L, H, indptr, indices, count, eff_len, groups, gtmask)
    m_idx = masked_structure(L, H, indptr, indices, gtmask)[1]
    cnt = np.ones(R) if count is None else count
    for model in (1, 2, 3, 4):
        want = posterior(cpu, post[f"m{model}_theta_before"], model)
        per_read = np.zeros(R)
        for h in range(H):
            ref = post[f"m{model}_post{h}"]
            assert ref.shape == want[h].shape == m_idx[h].shape
            np.testing.assert_allclose(want[h], ref, rtol=1e-12, atol=1e-300)
            np.add.at(per_read, m_idx[h].astype(np.int64), ref)
        touched = np.zeros(R, dtype=bool)
        for h in range(H):
            touched[m_idx[h]] = True
        np.testing.assert_allclose(per_read[touched], 1.0, rtol=1e-12)
    # model 4: the posteriors add up to the expected counts the same run reported
    got = np.zeros((H, L))
    m_ptr = masked_structure(L, H, indptr, indices, gtmask)[0]
    for h in range(H):
        col = np.repeat(np.arange(L), np.diff(m_ptr[h].astype(np.int64)))
        np.add.at(got[h], col, cnt[m_idx[h].astype(np.int64)] * post[f"m4_post{h}"])
    np.testing.assert_allclose(got, post["m4_expected_counts"], rtol=1e-12, atol=1e-300)


def _small_apm():
    from gbrs_amd.alignment import AlignmentPropertyMatrix
    g = load_golden(os.path.join(GOLD, "emmodel_m1_h2_count.npz"))
    R, L, H, indptr, indices, count, eff_len, groups, gtmask, values = fixture_inputs(g)
    return AlignmentPropertyMatrix(shape=(L, H, R), indptr=indptr, indices=indices, count=count,
                                   haplotype_names=[chr(65 + h) for h in range(H)],
                                   locus_names=[f"T{l:07d}" for l in range(L)])


def _provider(apm, asked):
    rng = np.random.default_rng(11)
    vals = [rng.random(len(ix)) + 0.5 for ix in apm.indices]

    def give(h):
        asked.append(h)
        return vals[h]
    return vals, give


@pytest.mark.parametrize("kind", ["callable", "sequence"])
def test_h5_value_provider_round_trip(tmp_path, kind):
    from gbrs_amd import emase_h5
    from gbrs_amd.alignment import load_alignment
    try:
        emase_h5._load()
    except (OSError, ImportError) as e:
        pytest.skip(str(e))
    apm = _small_apm()
    asked = []
    vals, give = _provider(apm, asked)
    path = str(tmp_path / "post.h5")
    emase_h5.save(apm, path, incidence_only=False, values=give if kind == "callable" else vals)
    if kind == "callable":
        assert asked == list(range(apm.num_haplotypes))          # one haplotype at a time, in order, once each
    back = load_alignment(path)
    assert back.shape == apm.shape and back.values is not None and apm.values is None
    for h in range(apm.num_haplotypes):
        assert np.array_equal(back.indptr[h], apm.indptr[h]) and np.array_equal(back.indices[h], apm.indices[h])
        assert np.array_equal(back.values[h], vals[h])
    assert np.array_equal(back.count, apm.count)
    # through the container's own save, and a provider of the wrong length is refused
    apm.save(str(tmp_path / "post2.h5"), incidence_only=False, values=give)
    assert np.array_equal(load_alignment(str(tmp_path / "post2.h5")).values[1], vals[1])
    with pytest.raises(RuntimeError, match="do not match"):
        emase_h5.save(apm, str(tmp_path / "bad.h5"), incidence_only=False, values=lambda h: vals[h][:-1])
    with pytest.raises(RuntimeError, match="number of value arrays"):
        emase_h5.save(apm, str(tmp_path / "bad.h5"), incidence_only=False, values=vals[:1])


@pytest.mark.parametrize("kind", ["callable", "sequence"])
def test_npz_value_provider_round_trip(tmp_path, kind):
    from gbrs_amd.alignment import load_alignment
    apm = _small_apm()
    asked = []
    vals, give = _provider(apm, asked)
    path = str(tmp_path / "post.npz")
    apm.save(path, values=give if kind == "callable" else vals)
    if kind == "callable":
        assert asked == list(range(apm.num_haplotypes))
    with np.load(path) as z:                                     # an ordinary .npz
        assert np.array_equal(z["values1"], vals[1]) and np.array_equal(z["indices0"], apm.indices[0])
    back = load_alignment(path)
    assert back.shape == apm.shape and back.hname == apm.hname and back.lname == apm.lname
    for h in range(apm.num_haplotypes):
        assert np.array_equal(back.indptr[h], apm.indptr[h]) and np.array_equal(back.indices[h], apm.indices[h])
        assert np.array_equal(back.values[h], vals[h])
    assert np.array_equal(back.count, apm.count)
    # without a provider the file is what it was before the argument existed
    apm.save(str(tmp_path / "plain.npz"))
    assert load_alignment(str(tmp_path / "plain.npz")).values is None


def test_parser_accepts_posterior_values(tmp_path):
    from gbrs_amd.cli import build_parser
    aln = tmp_path / "a.npz"
    aln.write_bytes(b"")
    args = build_parser().parse_args(["quantify", "-i", str(aln), "--posterior-values"])
    assert args.posterior_values is True and args.report_posterior is False
    args = build_parser().parse_args(["quantify", "-i", str(aln), "-w"])
    assert args.posterior_values is False and args.report_posterior is True
    text = build_parser()._subparsers._group_actions[0].choices["quantify"].format_help()
    assert "--posterior-values" in text and "incidence_only" in text


def test_quantify_refuses_merged_rows_before_any_device_call(tmp_path, monkeypatch):
    from gbrs_amd import _lib, quantify as q

    def no_device(*a, **kw):
        raise AssertionError("the device was touched")
    monkeypatch.setattr(_lib, "load", no_device)
    monkeypatch.setattr(_lib, "warm_up_device_async", no_device)
    monkeypatch.setattr(q, "load_alignment", no_device)
    with pytest.raises(RuntimeError, match=r"--posterior-values.*--merge-identical-rows"):
        q.quantify(str(tmp_path / "missing.npz"), outbase=str(tmp_path / "out"), posterior_values=True,
                   merge_identical_rows=True)
    assert os.listdir(tmp_path) == []


def test_sharded_launcher_refuses_posterior_values():
    from gbrs_amd.sharded import check_args
    base = dict(gpus=2, multiread_model=4, report_posterior=False, merge_identical_rows=False, devices=None, device=0,
                dist_backend="nccl")
    with pytest.raises(RuntimeError, match="--posterior-values"):
        check_args(argparse.Namespace(**base, posterior_values=True))
    with pytest.raises(RuntimeError, match="--report-posterior"):
        check_args(argparse.Namespace(**{**base, "report_posterior": True}, posterior_values=False))
    assert check_args(argparse.Namespace(**base, posterior_values=False)) == [0, 1]
