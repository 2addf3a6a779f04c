"""`bench.py --gpus N` means N ranks: without a launcher it starts torch.distributed.run with N
processes itself; under a launcher whose WORLD_SIZE differs from N it fails instead of timing fewer GPUs. The
multi-rank config-4 step (shard.partitioned_step, the code bench.py runs over RCCL) is checked here on CPU with gloo
at world 2: the ranks' outputs in rank order equal the world-1 output, on bench.py's own synthetic stream. The
per-rank matcher is the CPU oracle (this checks the sharding of the step; the kernels are checked in the -m gpu
tests). Also here: a plain run carries no side line, `--full` keeps them all, and `--dump-outputs` writes the last
step's outputs (whole, or the same seeded sample on every run)."""
import ctypes
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, K, DIV = 100_000, 3000, 10


def test_launch_command_rules():
    assert bench.launch_command(1, [], {}) is None
    assert bench.launch_command(8, [], {"WORLD_SIZE": "8"}) is None
    with pytest.raises(SystemExit):
        bench.launch_command(8, [], {"WORLD_SIZE": "1"})
    cmd = bench.launch_command(4, ["--gpus", "4", "--steps", "3"], {}, port=29999)
    assert cmd[1:4] == ["-m", "torch.distributed.run", "--nnodes=1"]
    assert "--nproc-per-node=4" in cmd and "127.0.0.1" in cmd and "--master-port=29999" in cmd
    assert cmd[-4:] == ["--gpus", "4", "--steps", "3"]


def _env(**kw):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR",
                                                             "MASTER_PORT")}
    env.update(kw)
    return env


@pytest.mark.timeout(300)
def test_bench_starts_its_ranks():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2"], env=_env(SM_BENCH_PROBE="1"),
                         capture_output=True, text=True, timeout=280)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [json.loads(x) for x in out.stdout.splitlines() if x.startswith("{")]
    assert sorted(d["rank"] for d in lines) == [0, 1]
    assert all(d["world"] == 2 and d["gpus"] == 2 for d in lines)


@pytest.mark.timeout(120)
def test_bench_refuses_world_mismatch():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "4"],
                         env=_env(WORLD_SIZE="2", RANK="0", SM_BENCH_PROBE="1"), capture_output=True, text=True,
                         timeout=110)
    assert out.returncode != 0
    assert "WORLD_SIZE=2" in out.stderr


def oracle_match(cols, ords):
    """The CPU oracle as a rank's matcher: packed (e2 << 32) | e1 global-ordinal tuples in its output order."""
    from oracle_lib import OracleApp, lib as olib
    sym, price, ts = (c.numpy() for c in cols)
    o = np.arange(len(ts), dtype=np.int64) if ords is None else ords.numpy()
    cs = [np.ascontiguousarray(sym), np.ascontiguousarray(price), np.zeros(len(ts), dtype=np.int64),
          np.ascontiguousarray(o)]
    a = OracleApp(bench.APP)
    a.start()
    ptrs = (ctypes.c_void_p * 4)(*[c.ctypes.data for c in cs])
    err = ctypes.create_string_buffer(512)
    tsa = np.ascontiguousarray(ts, dtype=np.int64)
    rc = olib().cr_send_columns(a.h, a.stream_index("StockStream"), len(tsa), tsa.ctypes.data, ptrs, err, 512)
    assert rc == 0, err.value
    out = a.outputs()["streams"].get("OutputStream", [])
    a.close()
    p = np.array([r[1] for r in out], dtype=np.int64).reshape(-1, 2)  # the selected e1 / e2 timestamp attributes
    return torch.from_numpy((p[:, 1] << 32) | p[:, 0])


def _rank(rank, world, port, outfile):
    from siddhi_amd.shard import partitioned_step
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        lo, hi = N * rank // world, N * (rank + 1) // world
        sym, price, vol, tsa, ts = bench.gen_stock(lo, hi, K, DIV, torch.device("cpu"), bench.seed_for(4))
        mine = partitioned_step(sym, [sym, price, ts], world, lo, N, oracle_match)
        parts = [None] * world
        dist.all_gather_object(parts, mine.tolist())
        if rank == 0:
            with open(outfile, "w") as f:
                json.dump(parts, f)
    finally:
        dist.destroy_process_group()


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


@pytest.mark.timeout(300)
def test_partitioned_step_world2_equals_world1(tmp_path):
    from siddhi_amd.shard import partitioned_step
    out = str(tmp_path / "parts.json")
    mp.start_processes(_rank, args=(2, _free_port(), out), nprocs=2, join=True, start_method="spawn")
    parts = json.load(open(out))
    sym, price, vol, tsa, ts = bench.gen_stock(0, N, K, DIV, torch.device("cpu"), bench.seed_for(4))
    single = partitioned_step(sym, [sym, price, ts], 1, 0, N, oracle_match)
    assert single.numel() > 0.3 * N
    got = np.concatenate([np.asarray(p, dtype=np.int64) for p in parts])
    np.testing.assert_array_equal(got, single.numpy())


def test_default_multi_gpu_plan_is_the_exchanged_stream():
    """`bench.py --gpus N` (config 4, no flags) measures BASELINE's configuration, one stream of N
    events routed by key over RCCL: value counts N (strong scaling), not N x world."""
    args = bench.build_parser().parse_args(["--gpus", "2"])
    assert args.config == 4 and not args.key_partitions
    plan = bench.run_plan(args.config, 2, env={})
    assert plan == {"shards": True, "units_factor": 1, "backend": "nccl", "exchange": True, "scaling": "strong"}
    for c in (2, 5):
        p = bench.run_plan(c, 8, env={})
        assert p["units_factor"] == 1 and p["backend"] == "nccl"
    assert bench.run_plan(5, 8, env={})["exchange"]
    # config 3 does not shard: replicas, counted per rank
    p3 = bench.run_plan(3, 4, env={})
    assert p3["units_factor"] == 4 and p3["scaling"] == "weak" and not p3["exchange"]
    assert bench.run_plan(4, 1, env={})["backend"] is None
    assert bench.run_plan(4, 2, env={"SM_BENCH_BACKEND": "gloo"})["backend"] == "gloo"


def test_stale_pmc_profile_yields_null_traffic(tmp_path, monkeypatch):
    """the roofline's PMC traffic is reported only when the committed summary names the same
    event count, query variant and library build (sm_build_id) as the running bench."""
    monkeypatch.setattr(bench, "ROOT", str(tmp_path))
    (tmp_path / "profiles").mkdir()
    n, m = 1000, 400
    ktot = {"stack": [10.0, 5], "order": [2.0, 5]}
    doc = {"config": 4, "events": n, "matches": m, "tag": "t", "build_id": "abcd", "variant": "literal",
           "method": "x", "labels": {"stack": {"hbm_bytes": 5e4}, "order": {"hbm_bytes": 1e4}}}
    (tmp_path / "profiles" / "pmc_config4.json").write_text(json.dumps(doc))
    r = bench.roofline(ktot, n, m, 5, 4, build_id="abcd")
    assert r["traffic"] == 5e4 and r["traffic_step"] == 6e4 and "build abcd" in r["traffic_source"]
    r = bench.roofline(ktot, n, m, 5, 4, build_id="ffff")
    assert r["traffic"] is None and r["traffic_step"] is None and "stale" in r["traffic_source"]
    r = bench.roofline(ktot, n + 1, m, 5, 4, build_id="abcd")
    assert r["traffic"] is None
    # a variant reads its own file; the literal query's profile never stands in for it
    r = bench.roofline(ktot, n, m, 5, 4, build_id="abcd", variant="pattern_count_not5s")
    assert r["traffic"] is None and "no profiles/pmc_config4_pattern_count_not5s.json" in r["traffic_source"]
    doc["variant"] = "pattern_count_not5s"
    (tmp_path / "profiles" / "pmc_config4_pattern_count_not5s.json").write_text(json.dumps(doc))
    assert bench.roofline(ktot, n, m, 5, 4, build_id="abcd", variant="pattern_count_not5s")["traffic"] == 5e4


def test_plain_run_is_the_default_and_full_is_opt_in():
    """A plain `bench.py --gpus 1 --steps K --warmup W` times its steps only; the side lines that take runs of their
    own (CPU baseline, H2D, sparse keys, input handler) wait for --full."""
    ap = bench.build_parser()
    plain = ap.parse_args(["--gpus", "1", "--steps", "3", "--warmup", "1"])
    assert not plain.full and plain.dump_outputs is None and plain.steps == 3 and plain.warmup == 1
    full = ap.parse_args(["--full", "--dump-outputs", "d"])
    assert full.full and full.dump_outputs == "d"


def test_dump_outputs_whole_and_sampled(tmp_path):
    """--dump-outputs: float64 .npy files; packed tuples become (e1, e2) columns; an output over the 64 MB budget is
    written as the same seeded, sorted sample of rows on every run, with its row indices and the full row count."""
    e1 = torch.arange(10, dtype=torch.int64) + 100
    e2 = torch.arange(10, dtype=torch.int64) + 3_000_000_000  # above 2^31: the high word is read unsigned
    d = str(tmp_path / "small")
    bench.write_outputs(d, "matches", (e2 << 32) | e1, True)
    got = np.load(os.path.join(d, "matches.npy"))
    assert got.dtype == np.float64 and got.shape == (10, 2)
    np.testing.assert_array_equal(got, np.stack([e1.numpy(), e2.numpy()], axis=1))
    assert np.load(os.path.join(d, "matches_count.npy")).tolist() == [10]
    assert not os.path.exists(os.path.join(d, "matches_index.npy"))
    bench.write_outputs(d, "records", torch.arange(60, dtype=torch.int64).reshape(5, 12), False, suffix=".rank1")
    assert np.load(os.path.join(d, "records.rank1.npy")).shape == (5, 12)

    n = 3_000_000  # 48 MB of (e1, e2) + nothing else would fit; with the indices it does not
    big = (torch.arange(n, dtype=torch.int64) << 32) | 7
    dirs = [str(tmp_path / x) for x in "ab"]
    for x in dirs:
        bench.write_outputs(x, "matches", big, True)
    files = sorted(os.listdir(dirs[0]))
    assert files == ["matches.npy", "matches_count.npy", "matches_index.npy"]
    assert sum(os.path.getsize(os.path.join(dirs[0], f)) for f in files) <= 64_000_000
    a = {f: np.load(os.path.join(dirs[0], f)) for f in files}
    for f in files:
        np.testing.assert_array_equal(a[f], np.load(os.path.join(dirs[1], f)))
    idx = a["matches_index.npy"]
    assert a["matches_count.npy"].tolist() == [n] and 2_000_000 < idx.size < n
    assert (np.diff(idx) >= 0).all() and idx[0] >= 0 and idx[-1] < n
    np.testing.assert_array_equal(a["matches.npy"], np.stack([np.full(idx.size, 7.0), idx], axis=1))


def _bench_line(extra, timeout=280):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--events", str(N), "--keys",
                        str(K), "--ts-div", str(DIV), "--steps", "2", "--warmup", "1"] + extra, env=_env(),
                       capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stderr[-3000:]
    js = [json.loads(x) for x in r.stdout.splitlines() if x.startswith("{")]
    assert len(js) == 1
    return js[0]


SIDE_LINES = ("e2e_with_h2d", "via_input_handler", "sparse_keys")


@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_plain_bench_dumps_the_oracle_matches(tmp_path):
    """The plain run on the small stream of this file: the headline fields, no side line, and --dump-outputs holding
    the last step's match tuples, which are the CPU oracle's for the same stream, in its order."""
    d = str(tmp_path / "out")
    line = _bench_line(["--dump-outputs", d])
    assert line["steps"] == 2 and line["warmup"] == 1 and not line["full"]
    assert line["unit"] == "events/s" and line["higher_is_better"] is True and line["dtype"] == "f64"
    assert abs(line["value"] - N / (line["ms_per_step"] * 1e-3)) < 1e-6 * line["value"]
    assert line["cpu_baseline"] is None and not any(k in line for k in SIDE_LINES)
    sym, price, vol, tsa, ts = bench.gen_stock(0, N, K, DIV, torch.device("cpu"), bench.seed_for(4))
    want = oracle_match([sym, price, ts], None).numpy()
    got = np.load(os.path.join(d, "matches.npy"))
    assert got.dtype == np.float64 and sorted(os.listdir(d)) == ["matches.npy", "matches_count.npy"]
    assert line["config"]["matches"] == len(want) == got.shape[0] > 0.3 * N
    np.testing.assert_array_equal(got, np.stack([want & 0xFFFFFFFF, want >> 32], axis=1))


@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_full_bench_keeps_its_side_lines():
    line = _bench_line(["--full", "--cpu-sample", "20000"])
    assert line["full"] and all(line[k]["value"] > 0 for k in SIDE_LINES)
    assert line["cpu_baseline"]["value"] > 0 and "oracle/cpu_ref" in line["cpu_baseline"]["sample"]
    assert line["via_input_handler"]["output_events"] == line["config"]["matches"] > 0
