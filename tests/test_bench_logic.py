"""bench.py's timed region (CPU only): W warmup steps then exactly K timed steps, twice - cold, then behind the pre-roll - and
what the line reports about it."""
import os
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _args(**kw):
    a = types.SimpleNamespace(steps=20, warmup=5, preroll_ms=40.0)
    a.__dict__.update(kw)
    return a


def test_timed_region_counts_steps_and_reports_both_regions():
    import bench
    calls, barriers = [], []

    def run_steps(k):
        calls.append(k)
        time.sleep(k * 1e-4)            # 0.1 ms per step

    dt, region = bench.timed_region(_args(), run_steps, lambda: barriers.append(len(calls)), 1, None, None, "cpu")
    # cold region: 5 + 20; pre-roll: ~40 ms / 0.1 ms; reported region: 5 + 20 again
    assert calls[0] == 5 and calls[1] == 20 and calls[3] == 5 and calls[4] == 20 and len(calls) == 5
    assert 10 <= calls[2] <= 450                        # (sleep granularity and a busy host make a step look longer than 0.1 ms)
    assert region["preroll"]["steps"] == calls[2] and region["preroll"]["asked_ms"] == 40.0
    assert region["cold_start"]["unit"] == "iters/s" and region["cold_start"]["ms_per_step"] > 0
    assert 20 * 0.9e-4 <= dt <= 20 * 1e-3               # the K steps of the second region only
    # a barrier on both sides of each timed region and behind the pre-roll
    assert barriers == [1, 2, 3, 4, 5]


def test_timed_region_without_preroll_is_the_old_form():
    import bench
    calls = []
    dt, region = bench.timed_region(_args(preroll_ms=0.0, steps=7, warmup=2), lambda k: calls.append(k), lambda: None, 1, None, None,
                                    "cpu")
    assert calls == [2, 7] and region is None and dt >= 0.0


def test_timed_region_reset_puts_the_reported_region_back_at_the_start():
    """The reported region computes the same W + K iterations as the cold one, however many steps the pre-roll took."""
    import bench
    events = []

    def run_steps(k):
        events.append(("steps", k))
        time.sleep(k * 1e-4)

    dt, region = bench.timed_region(_args(), run_steps, lambda: events.append(("barrier",)), 1, None, None, "cpu",
                                    reset=lambda: events.append(("reset",)))
    n_pre = region["preroll"]["steps"]
    assert events == [("steps", 5), ("barrier",), ("steps", 20), ("barrier",), ("steps", n_pre), ("barrier",), ("reset",),
                      ("steps", 5), ("barrier",), ("steps", 20), ("barrier",)]
    calls = []
    bench.timed_region(_args(preroll_ms=0.0), calls.append, lambda: None, 1, None, None, "cpu",
                       reset=lambda: calls.append("reset"))
    assert calls == [5, 20]                             # without a pre-roll the only region starts from the prepared state


def test_parse_steps_and_dump_outputs(monkeypatch):
    import pytest

    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "3", "--dump-outputs", "out"])
    a = bench.parse()
    assert (a.gpus, a.steps, a.warmup, a.dump_outputs) == (1, 7, 3, "out")
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "9"])
    assert bench.parse().dump_outputs is None
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "0"])
    with pytest.raises(SystemExit):
        bench.parse()


def test_parse_full_is_off_unless_asked(monkeypatch):
    """A plain run times the headline alone; --full adds the rest, and the --no-* switches still pick parts of it."""
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "3"])
    assert bench.parse().full is False
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--no-hmm", "--steps", "7"])
    a = bench.parse()
    assert a.full and a.no_hmm and not a.no_check and a.steps == 7


def test_dump_outputs_writes_float64_files(tmp_path):
    import numpy as np

    import bench
    theta = np.random.default_rng(1).random((8, 100))
    calls = np.arange(50, dtype=np.int32).reshape(1, 50)
    written = bench.dump_outputs(str(tmp_path / "d"), {"em_theta": theta, "hmm_calls": calls})
    assert written == {"em_theta": (8, 100), "hmm_calls": (1, 50)}
    got = np.load(tmp_path / "d" / "em_theta.npy")
    assert got.dtype == np.float64 and np.array_equal(got, theta)
    got = np.load(tmp_path / "d" / "hmm_calls.npy")
    assert got.dtype == np.float64 and np.array_equal(got, calls)


def test_dump_outputs_samples_the_same_positions_under_the_size_cap(tmp_path):
    import numpy as np

    import bench
    big = {"a": np.arange(200_000, dtype=np.float64), "b": np.arange(100_000, dtype=np.int64).reshape(100, 1000)}
    limit = 1_200_000
    w1 = bench.dump_outputs(str(tmp_path / "1"), big, limit=limit)
    w2 = bench.dump_outputs(str(tmp_path / "2"), big, limit=limit)
    assert w1 == w2 and 0 < w1["a"][0] < 200_000 and 0 < w1["b"][0] < 100_000
    total = sum(os.path.getsize(tmp_path / "1" / f"{k}.npy") for k in big)
    assert total <= limit
    for k, v in big.items():
        s1, s2 = np.load(tmp_path / "1" / f"{k}.npy"), np.load(tmp_path / "2" / f"{k}.npy")
        assert s1.dtype == np.float64 and s1.ndim == 1 and 0 < s1.size < v.size
        assert np.array_equal(s1, s2)
        # a sample of the flat array at sorted positions: values of arange are their own positions
        assert np.all(np.diff(s1) > 0) and np.all(np.isin(s1, v.reshape(-1)))
