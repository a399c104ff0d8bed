"""bench.py's own rank launcher and the RCCL id rendezvous, on CPU (no GPU, no torch): `python bench.py --gpus N` must
start N ranks or fail -- never print a one-GPU line under an N-GPU name (round-3 review, row e)."""
import argparse
import json
import os
import subprocess
import sys
import textwrap
import time

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402


def _args(gpus):
    return argparse.Namespace(gpus=gpus)


def test_resolve_world_modes():
    assert bench.resolve_world(_args(1), environ={}) == ("single", 0, 1)
    assert bench.resolve_world(_args(4), environ={}, n_devices=8) == ("launch", 0, 4)
    assert bench.resolve_world(_args(4), environ={"RANK": "3", "WORLD_SIZE": "4"}) == ("rank", 3, 4)
    assert bench.resolve_world(_args(1), environ={"RANK": "0", "WORLD_SIZE": "1"}) == ("rank", 0, 1)
    with pytest.raises(SystemExit) as e:                               # fewer devices than asked for: refuse
        bench.resolve_world(_args(8), environ={}, n_devices=1)
    assert "needs 8 visible" in str(e.value) and "shows 1" in str(e.value)
    with pytest.raises(SystemExit) as e:                               # launcher and flag disagree: refuse
        bench.resolve_world(_args(2), environ={"RANK": "0", "WORLD_SIZE": "8"})
    assert "WORLD_SIZE=8" in str(e.value)
    with pytest.raises(SystemExit):                                    # the old silent case: --gpus 8 in a 1-rank environment
        bench.resolve_world(_args(8), environ={"RANK": "0", "WORLD_SIZE": "1"})


def test_gpus_2_without_devices_fails_with_a_clear_message():
    """The shape of the driver's command line on a box that cannot satisfy it (this container has no GPU at all)."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "5"], env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode != 0
    assert "needs 2 visible MI355X devices" in r.stderr
    assert "n_gpus" not in r.stdout                                    # no JSON line of a smaller job


STUB = textwrap.dedent('''
    import json, os, sys, time
    sys.path.insert(0, %(root)r)
    from commpy_amd.parallel import exchange_unique_id, shard_bounds
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    assert os.environ["LOCAL_RANK"] == os.environ["RANK"] and os.environ["MASTER_ADDR"] == "127.0.0.1"
    assert int(os.environ["MASTER_PORT"]) > 0 and len(os.environ["CPX_COMM_NONCE"]) == 32
    if rank == 1:
        time.sleep(%(late)f)                     # a rank that reaches the rendezvous long after rank 0 published the id
    blob = exchange_unique_id(rank, world, lambda: bytes([7]) * 128, timeout=60)      # default path: keyed by the nonce
    assert blob == bytes([7]) * 128
    lo, hi = shard_bounds(1000, rank, world)     # the stub "decode": every rank reports its shard
    open(os.path.join(%(out)r, "rank%%d.json" %% rank), "w").write(json.dumps({"rank": rank, "rows": [lo, hi],
                                                                               "nonce": os.environ["CPX_COMM_NONCE"]}))
    if rank == %(fail)d:
        sys.exit(3)
    if %(hang)d and rank != 0:
        time.sleep(600)                          # would wait for the failed rank in a collective
    if rank == 0:
        print(json.dumps({"n_gpus": world}), flush=True)
''')


def _stub(tmp_path, late=0.0, fail=-1, hang=0):
    path = tmp_path / "stub.py"
    path.write_text(STUB % {"root": ROOT, "out": str(tmp_path), "late": late, "fail": fail, "hang": hang})
    return [sys.executable, str(path)]


def test_launch_ranks_starts_n_ranks_with_a_per_launch_nonce(tmp_path, capfd):
    rc = bench.launch_ranks(4, _stub(tmp_path, late=3.0), timeout=120)
    assert rc == 0
    got = [json.load(open(tmp_path / ("rank%d.json" % r))) for r in range(4)]
    assert [g["rows"] for g in got] == [[0, 250], [250, 500], [500, 750], [750, 1000]]
    assert len({g["nonce"] for g in got}) == 1
    assert json.loads(capfd.readouterr().out.strip().splitlines()[-1]) == {"n_gpus": 4}    # rank 0's line passes through
    # a second launch gets another nonce (and so another id file)
    assert bench.launch_ranks(2, _stub(tmp_path), timeout=120) == 0
    assert json.load(open(tmp_path / "rank0.json"))["nonce"] != got[0]["nonce"]


def test_launch_ranks_propagates_a_failing_rank_and_stops_the_others(tmp_path):
    t0 = time.time()
    rc = bench.launch_ranks(3, _stub(tmp_path, fail=0, hang=1), timeout=120)
    assert rc == 3
    assert time.time() - t0 < 60                                       # the sleeping ranks were terminated, not waited for


def test_id_exchange_rejects_a_file_of_another_launch(tmp_path):
    """the freshness test compared an mtime with a procfs ctime.  Now a reader only accepts a file that carries
    its own launch's nonce -- whatever the clocks say."""
    from commpy_amd import parallel
    path = str(tmp_path / "id")
    # a leftover with the right magic but another launch's nonce, freshly written
    with open(path, "wb") as f:
        f.write(parallel._ID_MAGIC + b"other-launch\n" + b"\xee" * 128)
    with pytest.raises(TimeoutError) as e:
        parallel.exchange_unique_id(1, 2, None, path=path, timeout=0.3, nonce="this-launch")
    assert "another launch" in str(e.value)
    # rank 0 of this launch replaces it; a reader that arrives later (any delay) gets this launch's id
    assert parallel.exchange_unique_id(0, 2, lambda: b"\x11" * 128, path=path, nonce="this-launch") == b"\x11" * 128
    os.utime(path, (1.0e9, 1.0e9))                                     # an "old" mtime must not matter any more
    assert parallel.exchange_unique_id(1, 2, None, path=path, timeout=5, nonce="this-launch") == b"\x11" * 128
    # the nonce distinguishes launchers, ports, restarts and communicators of one job
    n0 = parallel.launch_nonce(0)
    assert parallel.launch_nonce(1) != n0
    old = os.environ.get("CPX_COMM_NONCE")
    try:
        os.environ["CPX_COMM_NONCE"] = "abc"
        assert parallel.launch_nonce(0).startswith("abc.") and parallel.launch_nonce(0) != n0
    finally:
        if old is None:
            del os.environ["CPX_COMM_NONCE"]
        else:
            os.environ["CPX_COMM_NONCE"] = old
    assert parallel._launcher_start_ticks().isdigit() and int(parallel._launcher_start_ticks()) > 0


def _bench_gpus_2_on_the_host_stand_in(tmp_path, *extra):
    """`bench.py --gpus 2 --steps 2 --warmup 1 --batch 48` against tests/fake_engine.py, two ranks started by bench.py's own
    launcher; returns rank 0's JSON line."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "CPX_COMM_NONCE")}
    env["CPX_FAKE_DIR"] = str(tmp_path)
    env["CPX_FAKE_DEVICES"] = "2"
    out_path = tmp_path / "stdout.txt"
    with open(out_path, "w") as fo:
        argv = [sys.executable, os.path.join(ROOT, "tests", "fake_engine.py"), "--gpus", "2", "--steps", "2", "--warmup", "1",
                "--batch", "48"] + list(extra)
        # bench.launch_ranks inherits stdout: run it in a child so that rank 0's line lands in a file
        code = ("import sys; sys.path.insert(0, %r); import bench; sys.exit(bench.launch_ranks(2, %r, timeout=240))" % (ROOT, argv))
        r = subprocess.run([sys.executable, "-c", code], env=env, stdout=fo, stderr=subprocess.PIPE, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in open(out_path).read().splitlines() if ln.startswith("{")]
    assert len(lines) == 1, lines                                      # ONE line, from rank 0
    return json.loads(lines[0])


def test_bench_gpus_2_end_to_end_against_the_host_stand_in(tmp_path):
    """`bench.py --gpus 2` has never run with two ranks on hardware (one GPU per lease; SCALE_r01..r04 skipped).  Here its rank
    path runs END TO END in two real processes started by bench.py's own launcher, against tests/fake_engine.py -- a host
    stand-in for the C-ABI that lives in tests/ only (the product has no CPU fallback): RankComm's nonce rendezvous,
    cpx_comm_init_rank -> allgather_dev -> allreduce -> cpx_comm_info, the in-place gather layout and its checksum exchange, and
    the N > 1 fields of the JSON line (the all-gather region and the checks are --full)."""
    j = _bench_gpus_2_on_the_host_stand_in(tmp_path, "--no-cpu-baseline", "--full")
    assert j["n_gpus"] == 2 and j["steps"] == 2 and j["scaling"] == "weak" and j["full"] is True
    assert j["config"]["batch_per_gpu"] == 48 and "x2" in j["config"]["parallelism"]
    assert j["config"]["collectives"] == "engine RCCL binding (cpx_comm_*)"
    assert j["value"] > 0 and j["value_with_gather"] > 0 and j["ms_per_step_with_gather"] > 0
    assert j["comm_world"] == {"nranks": 2, "this_rank": 0, "source": "ncclCommCount / ncclCommUserRank"}
    assert j["gather"]["all_slots_ok_on_all_ranks"] is True and j["gather"]["bytes_per_rank_per_step"] == 48 * 1030
    assert j["oracle_mismatched_bits"] == 0 and j["cpu_baseline"] is None and j["other_configs"] is None
    assert j["launcher"] == "bench.py (subprocess per rank)"
    assert 0.0 <= j["ber"] < 0.05
    for rank in (0, 1):
        calls = json.load(open(tmp_path / ("calls_rank%d.json" % rank)))
        for name in ("cpx_comm_init_rank", "cpx_comm_allgather_u8", "cpx_comm_allreduce_i64", "cpx_comm_allreduce_f64", "cpx_comm_info",
                     "cpx_comm_destroy"):
            assert name in calls, (rank, name)
        assert calls.index("cpx_comm_init_rank") < calls.index("cpx_comm_allgather_u8") < calls.index("cpx_comm_info")
        assert ("cpx_comm_unique_id" in calls) == (rank == 0)          # rank 0 makes the id, rank 1 reads it from the nonce-keyed file


def test_bench_gpus_2_plain_run_times_the_decode_and_nothing_else(tmp_path):
    """Without --full an N > 1 run forms the communicator, times the K decode steps (max over ranks) and prints the line: no
    all-gather region, no checks after it; the fields only --full fills are there as null."""
    j = _bench_gpus_2_on_the_host_stand_in(tmp_path)
    assert j["n_gpus"] == 2 and j["steps"] == 2 and j["full"] is False
    assert j["value"] > 0 and j["ms_per_step"] > 0 and j["unit"] == "info-bits/s" and j["higher_is_better"] is True
    assert j["dtype"] == "f64" and j["roofline"]["kernel_ms_avg"] > 0
    assert j["comm_world"] == {"nranks": 2, "this_rank": 0, "source": "ncclCommCount / ncclCommUserRank"}
    assert j["kernel_path_check"]["mismatching_bits_between_repeats"] == 0
    assert "all-gather" not in j["config"]["parallelism"]
    for key in ("value_with_gather", "ms_per_step_with_gather", "gather", "ber", "oracle_mismatched_bits", "oracle_sample_codewords",
                "demod_max_abs_err_vs_oracle", "other_configs", "cpu_baseline"):
        assert j[key] is None, key
    assert j["roofline"]["clock"] is None and j["roofline"]["sustained"] is None
    for rank in (0, 1):
        calls = json.load(open(tmp_path / ("calls_rank%d.json" % rank)))
        assert "cpx_comm_init_rank" in calls and "cpx_comm_allreduce_f64" in calls and "cpx_comm_destroy" in calls
        assert "cpx_comm_allgather_u8" not in calls, rank


def _bench_single_on_the_host_stand_in(tmp_path, *extra, opt_outs=True):
    """`bench.py --gpus 1` against tests/fake_engine.py (host stand-in for the C-ABI, tests/ only); returns (exit code, JSON line or
    None, stderr).  opt_outs: leave out the path check and what --full would add that the stand-in cannot serve or that takes
    seconds (cpu_baseline, other_configs, the sustained phase)."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "CPX_COMM_NONCE")}
    env["CPX_FAKE_DIR"] = str(tmp_path)
    env["CPX_FAKE_DEVICES"] = "1"
    argv = [sys.executable, os.path.join(ROOT, "tests", "fake_engine.py"), "--gpus", "1", "--batch", "40"]
    if opt_outs:
        argv += ["--no-cpu-baseline", "--no-other-configs", "--no-path-check", "--sustain-seconds", "0"]
    argv += list(extra)
    r = subprocess.run(argv, env=env, capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) <= 1, lines
    return r.returncode, (json.loads(lines[0]) if lines else None), r.stderr


def test_bench_dump_outputs_writes_the_timed_decode_and_is_reproducible(tmp_path):
    """--dump-outputs DIR: after the timed steps, the bits the last timed step decoded land in DIR as float32 / float64 .npy
    (a fixed, seeded sample of rows plus a checksum of every codeword), identical from run to run with the same arguments and
    with or without --full; --steps is the number of timed steps and the line carries ms_per_step."""
    import numpy as np
    runs = []
    for k, (steps, full) in enumerate(((3, []), (4, ["--full"]))):
        out_dir = tmp_path / ("dump%d" % k)
        code, j, err = _bench_single_on_the_host_stand_in(tmp_path, "--steps", str(steps), "--warmup", "1",
                                                          "--dump-outputs", str(out_dir), *full)
        assert code == 0, err[-2000:]
        assert j["steps"] == steps and j["ms_per_step"] > 0 and j["full"] is bool(full)
        assert j["oracle_mismatched_bits"] == (0 if full else None)    # the oracle sample is a check of --full
        assert sorted(j["dump_outputs"]["files"]) == ["decoded_bits.npy", "decoded_bits_rows.npy", "decoded_bits_weighted_sum.npy"]
        arrays = {f: np.load(out_dir / f) for f in j["dump_outputs"]["files"]}
        assert sum(a.nbytes for a in arrays.values()) <= 64 << 20
        assert all(a.dtype in (np.float32, np.float64) for a in arrays.values())
        runs.append(arrays)
    bits, rows, wsum = (runs[0][f] for f in ("decoded_bits.npy", "decoded_bits_rows.npy", "decoded_bits_weighted_sum.npy"))
    assert bits.shape == (40, 1030) and np.array_equal(rows, np.arange(40)) and wsum.shape == (40,)
    assert set(np.unique(bits)) <= {0.0, 1.0} and bits.sum() > 0
    assert np.array_equal(wsum, bits @ np.arange(1, 1031, dtype=np.float32))
    for f in runs[0]:
        assert np.array_equal(runs[0][f], runs[1][f]), f             # same inputs, same outputs, whatever the number of steps or --full
    # a larger batch than the sample: a seeded subset of rows, the same every time
    assert np.array_equal(bench.dump_sample_rows(65536), bench.dump_sample_rows(65536))
    assert len(bench.dump_sample_rows(65536)) == bench.DUMP_SAMPLE_CODEWORDS
    assert bench.dump_bytes(65536, 1030) <= bench.DUMP_LIMIT_BYTES


def test_bench_plain_run_leaves_out_what_only_full_adds(tmp_path):
    """Without --full and without any opt-out a one-GPU run sets up, runs the kernel-path check, warms up, times the steps and
    prints the line: none of the checks after the timed region, the clock probe, the sustained phase, `other_configs` (which
    the stand-in cannot serve) or `cpu_baseline` runs; their fields are null."""
    code, j, err = _bench_single_on_the_host_stand_in(tmp_path, "--steps", "2", "--warmup", "1", opt_outs=False)
    assert code == 0, err[-2000:]
    assert j["full"] is False and j["n_gpus"] == 1 and j["steps"] == 2 and j["warmup"] == 1
    assert j["value"] > 0 and j["ms_per_step"] > 0 and j["dtype"] == "f64" and j["unit"] == "info-bits/s"
    assert j["metric"] == "decoded info-bits/s at fixed Eb/N0 (Viterbi K=7 r=1/2, 1024b); BER match" and j["higher_is_better"] is True
    assert j["kernel_path_check"]["codewords"] == 40 and j["kernel_path_check"]["mismatching_bits_between_repeats"] == 0
    assert j["roofline"]["kernel"].startswith("viterbi_cw_fused_kernel") and j["roofline"]["kernel_ms_avg"] > 0
    for key in ("ber", "oracle_mismatched_bits", "oracle_sample_codewords", "demod_max_abs_err_vs_oracle", "other_configs", "cpu_baseline"):
        assert j[key] is None, key
    assert j["roofline"]["clock"] is None and j["roofline"]["sustained"] is None
    assert "dump_outputs" not in j


def test_bench_refuses_zero_steps(tmp_path):
    code, j, err = _bench_single_on_the_host_stand_in(tmp_path, "--steps", "0")
    assert code != 0 and j is None and "--steps" in err
