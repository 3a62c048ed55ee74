"""`gbrs quantify --gpus N` without a GPU: the flags, the refusals, the launch plan, and the per-rank driver over two gloo
ranks with the numpy stand-in engine (tests/cpu_engine.py) and gbrs_amd.dist.shard_rows in place of the device."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT


def _parse(argv):
    from gbrs_amd.cli import build_parser
    return build_parser().parse_args(argv)


@pytest.fixture
def aln_file(tmp_path):
    p = tmp_path / "in" / "aln.npz"
    p.parent.mkdir()
    p.write_bytes(b"")
    return str(p)


def test_parser_takes_the_sharding_flags(aln_file):
    a = _parse(["quantify", "-i", aln_file, "--gpus", "4", "--devices", "3,2,1,0", "--dist-backend", "gloo"])
    assert (a.gpus, a.devices, a.dist_backend) == (4, "3,2,1,0", "gloo")
    a = _parse(["quantify", "-i", aln_file])
    assert (a.gpus, a.devices, a.dist_backend) == (None, None, "nccl")
    with pytest.raises(SystemExit):
        _parse(["quantify", "-i", aln_file, "--gpus", "2", "--dist-backend", "mpi"])


REFUSED = [
    (["-M", "2"], "multiread model 2"),
    (["-M", "1"], "multiread model 1"),
    (["-w"], "report-posterior"),
    (["--merge-identical-rows"], "merge-identical-rows"),
    (["--devices", "0,1,2"], "names 3 devices"),
    (["--devices", "0,0"], "repeats a device"),
    (["--devices", "0,x"], "comma-separated"),
]


@pytest.mark.parametrize("extra,message", REFUSED)
def test_refusals_log_return_zero_and_start_nothing(tmp_path, aln_file, monkeypatch, caplog, extra, message):
    from gbrs_amd import cli
    started = []
    monkeypatch.setattr(subprocess, "Popen", lambda *a, **k: started.append(a) or pytest.fail("a child was started"))
    monkeypatch.delenv("GBRS_STAGE_TIMES", raising=False)
    out = tmp_path / "out"
    out.mkdir()
    argv = ["quantify", "-i", aln_file, "-o", str(out / "q"), "--gpus", "2"] + extra
    with caplog.at_level("ERROR", logger="gbrs"):
        assert cli.main(argv) == 0
    assert any(message in r.getMessage() for r in caplog.records if r.levelname == "ERROR"), caplog.text
    assert started == [] and os.listdir(out) == []


@pytest.mark.parametrize("n", ["0", "-1"])
def test_refuses_fewer_than_one_rank(tmp_path, aln_file, monkeypatch, caplog, n):
    from gbrs_amd import cli
    monkeypatch.setattr(subprocess, "Popen", lambda *a, **k: pytest.fail("a child was started"))
    with caplog.at_level("ERROR", logger="gbrs"):
        assert cli.main(["quantify", "-i", aln_file, "-o", str(tmp_path / "q"), "--gpus", n]) == 0
    assert "at least 1" in caplog.text
    assert [p for p in os.listdir(tmp_path) if p.startswith("q")] == []


def test_gloo_takes_a_repeated_device(aln_file):
    from gbrs_amd.sharded import check_args
    assert check_args(_parse(["quantify", "-i", aln_file, "--gpus", "2", "--devices", "0,0",
                              "--dist-backend", "gloo"])) == [0, 0]


def test_launch_plan(aln_file, monkeypatch):
    from gbrs_amd.sharded import launch_plan
    argv = ["quantify", "-i", aln_file, "--gpus", "3", "--device", "2"]
    env = {"PATH": "/bin", "GBRS_STAGE_TIMES": "/x.json"}
    monkeypatch.setattr(os, "sched_getaffinity", lambda pid: set(range(64)), raising=False)
    plan = launch_plan(_parse(argv), argv, 4242, environ=env)
    assert len(plan) == 3
    for k, (cmd, e) in enumerate(plan):
        assert cmd == [sys.executable, "-m", "gbrs_amd.sharded"] + argv
        assert (e["RANK"], e["WORLD_SIZE"], e["LOCAL_RANK"]) == (str(k), "3", str(k))
        assert (e["MASTER_ADDR"], e["MASTER_PORT"]) == ("127.0.0.1", "4242")
        assert e["GBRS_SHARD_DEVICE"] == str(2 + k) and e["GBRS_SHARD_BACKEND"] == "nccl"
        assert e["GBRS_IO_THREADS"] == str(32 // 3)          # min(32, affinity) split over the ranks
        assert e["PYTHONPATH"].split(os.pathsep)[0] == ROOT
        assert "GBRS_STAGE_TIMES" not in e                    # the launcher gives every rank a file of its own
    # explicit devices and a user's thread count are kept
    argv = ["quantify", "-i", aln_file, "--gpus", "2", "--devices", "5,1", "--dist-backend", "gloo"]
    plan = launch_plan(_parse(argv), argv, 1, environ={"GBRS_IO_THREADS": "7"})
    assert [e["GBRS_SHARD_DEVICE"] for _, e in plan] == ["5", "1"]
    assert [e["GBRS_IO_THREADS"] for _, e in plan] == ["7", "7"]
    assert [e["GBRS_SHARD_BACKEND"] for _, e in plan] == ["gloo", "gloo"]


def test_launch_stops_the_other_ranks_when_one_fails(aln_file, monkeypatch, caplog):
    """A rank that exits non-zero: the others are terminated, the failure is logged with the rank's last line, 0."""
    from gbrs_amd import cli, sharded
    script = ("import os, sys, time\n"
              "r = int(os.environ['RANK'])\n"
              "if r == 1:\n"
              "    sys.stderr.write('rank one gives up\\n'); sys.exit(3)\n"
              "time.sleep(60)\n")

    def plan(args, argv, port, environ=None):
        return [([sys.executable, "-c", script], dict(os.environ, RANK=str(k))) for k in range(args.gpus)]
    monkeypatch.setattr(sharded, "launch_plan", plan)
    started = []
    real = subprocess.Popen

    def popen(*a, **k):
        started.append(real(*a, **k))
        return started[-1]
    monkeypatch.setattr(subprocess, "Popen", popen)
    with caplog.at_level("ERROR", logger="gbrs"):
        assert cli.main(["quantify", "-i", aln_file, "--gpus", "3", "--devices", "0,1,2"]) == 0
    assert "rank 1 of 3 failed (exit status 3): rank one gives up" in caplog.text
    assert len(started) == 3 and all(p.poll() is not None for p in started)


# ---- the per-rank driver on two gloo ranks, numpy engine --------------------------------------------------------

def _rank_worker(rank, world, port, argv, out):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch
    import torch.distributed as dist
    from cpu_engine import NumpyEngine
    from gbrs_amd import sharded
    from gbrs_amd.cli import build_parser
    from gbrs_amd.dist import PipelinedShardedEM, ShardedEM, shard_rows, split_at_locus

    class Done:
        def wait(self):
            pass

    class NumpyOps:
        device = 0

        def min_all(self, v):
            t = torch.tensor([int(v)])
            dist.all_reduce(t, op=dist.ReduceOp.MIN)
            return int(t.item())

        def shard(self, aln, rank, world, l_split):
            L, H, R = aln.shape
            bounds = [shard_rows(aln.indptr, aln.indices, None, R, k, world)[0] for k in range(world)] + [R]
            sharded.check_blocks(bounds)
            r0, r1, ip, ix, cnt = shard_rows(aln.indptr, aln.indices, aln.count, R, rank, world)
            straddling, sides = 0, (0, 0)
            if l_split:
                (a_ip, a_ix), (b_ip, b_ix) = split_at_locus(ip, ix, l_split)
                in_a, in_b = np.zeros(r1 - r0, bool), np.zeros(r1 - r0, bool)
                for x in a_ix:
                    in_a[x] = True
                for x in b_ix:
                    in_b[x] = True
                straddling = int((in_a & in_b).sum())
                sides = (sum(map(len, a_ix)), sum(map(len, b_ix)))
            return sharded.Shard(r0, r1, bounds, straddling, sides, dict(ip=ip, ix=ix, cnt=cnt))

        def engines(self, shard, L, H, eff, allowed, l_split):
            d, R = shard.data, shard.r1 - shard.r0
            if not l_split:
                return [NumpyEngine(R, L, H, d["ip"], d["ix"], d["cnt"], eff)]
            (a_ip, a_ix), (b_ip, b_ix) = split_at_locus(d["ip"], d["ix"], l_split)
            return [NumpyEngine(R, l_split, H, a_ip, a_ix, d["cnt"], None if eff is None else eff[:, :l_split]),
                    NumpyEngine(R, L - l_split, H, b_ip, b_ix, d["cnt"], None if eff is None else eff[:, l_split:])]

        def driver(self, engs):
            if len(engs) == 1:
                return ShardedEM(engs[0], lambda arr, n: dist.all_reduce(torch.from_numpy(arr)))
            return PipelinedShardedEM(engs[0], engs[1], lambda arr, n: dist.all_reduce(torch.from_numpy(arr)) or Done())

        def results(self, drv, engs):
            return (np.concatenate([e.theta for e in engs], axis=1), np.concatenate([e.counts for e in engs], axis=1))

        def close(self, engs):
            pass

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    marks = {}
    sharded.run_rank(build_parser().parse_args(argv), rank, world, NumpyOps(), marks, backend="gloo")
    np.save(os.path.join(out, f"marks{rank}.npy"), np.array([marks["path"], marks["em_iterations"]], dtype=object),
            allow_pickle=True)
    dist.destroy_process_group()


@pytest.mark.parametrize("name,path", [("h8_count_len", "two-engine"), ("h8_pseudo", "single-engine"),
                                       ("h2_len", "two-engine")])
def test_rank_driver_two_gloo_ranks(tmp_path, name, path):
    import torch.multiprocessing as mp
    from sharded_cases import check_reports_against_golden, write_case
    argv, suffix, g, _ = write_case(tmp_path, name)
    argv += ["-o", str(tmp_path / "out"), "--gpus", "2", "--dist-backend", "gloo"]
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    mp.spawn(_rank_worker, args=(2, port, argv, str(tmp_path)), nprocs=2, join=True)
    for k in range(2):
        got_path, n = np.load(tmp_path / f"marks{k}.npy", allow_pickle=True)
        assert got_path == path and int(n) == int(g["num_iters"])
    check_reports_against_golden(tmp_path / f"out.{suffix}", g)
