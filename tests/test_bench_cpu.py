"""CPU: bench.py's launch contract and its N > 1 branch, end to end to the JSON line (that branch had never run
anywhere, and `python bench.py --gpus N` without torch.distributed.run printed nothing), as a plain run and with --full."""
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
DRIVER = os.path.join(HERE, "bench_world2_driver.py")
ARGS = ["--gpus", "2", "--rows", "6001", "--batch", "16", "--steps", "2", "--warmup", "1"]


def _strict(text: str) -> dict:
    def bad(c):
        raise ValueError(f"non-finite constant {c} in the bench line")
    return json.loads(text, parse_constant=bad)


def _line(out: str) -> dict:
    lines = out.splitlines()
    assert len(lines) == 1, out[-3000:]                      # stdout holds exactly ONE line (rank 0's JSON) and nothing else
    assert len(lines[0].encode()) <= 8192, len(lines[0])     # a 23-KB line was not parsed by the driver
    return _strict(lines[0])


def _check(o, full=True):
    assert o["full"] is full
    assert o["n_gpus"] == 2 and o["steps"] == 2 and o["warmup"] == 1 and o["scaling"] == "strong" and o["higher_is_better"] is True
    c = o["config"]
    assert c["n_ranks_seen"] == 2 and c["rows"] == 6001 and c["rows_per_rank"] == 3001 and c["parallelism"].startswith("row-shard x2")
    assert "all_gather_into_tensor" in c["exchange"]        # gloo: the torch.distributed exchange (the RCCL one needs GPUs)
    assert o["value"] > 0 and abs(o["value"] - 16 / (o["ms_per_step"] * 1e-3)) / o["value"] < 1e-3
    assert o["secondary"] == [] and o["cpu_baseline"] is None      # N > 1: the headline only
    assert o["dtype"] == "f32"                                     # the oracle-backed index answers on the exact path
    if full:
        # the merged answer is the global one: every planted neighbour (all in rank 0's shard) is the top hit, lists are sorted,
        # and the default and exact paths agree on every rank (MIN over ranks)
        assert o["planted_top1"] == 1.0 and o["sorted"] is True and o["identical_to_exact_f32_scan"] is True
        assert o["roofline"]["kernel_ms"] == 1.0 and o["full_record"] == "bench_secondary.json"
    else:
        # a plain run: set-up, warm-up, timed steps, the line -- no checks, no kernel timing, no full record
        for k in ("planted_top1", "sorted", "identical_to_exact_f32_scan", "recall_at_10", "roofline", "full_record"):
            assert o[k] is None, k


def test_world2_under_torch_distributed_run():
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                        "--master-port", str(port), DRIVER, *ARGS, "--full"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    _check(_line(r.stdout))
    assert "[bench] full record: " in r.stderr


def test_plain_run_times_the_headline_only():
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, DRIVER, *ARGS], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    _check(_line(r.stdout), full=False)
    assert "[bench] " not in r.stderr                             # no legs, no full record


def test_plain_python_invocation_self_launches_its_ranks():
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    r = subprocess.run([sys.executable, DRIVER, *ARGS, "--full"], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    o = _line(r.stdout)
    _check(o)
    assert o["config"]["self_launched"] is True


def test_mismatched_world_size_is_refused():
    env = dict(os.environ, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0")
    r = subprocess.run([sys.executable, DRIVER, *ARGS], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 2 and "must agree" in r.stderr


def test_compact_line_bounds_a_real_full_record():
    """The stdout line built from round 5's real 23-KB record (14 secondary legs): <= 8 KB, strict JSON, every key the bench
    contract and the tier's measurement section name; the full record goes to bench_secondary.json, not to stdout."""
    sys.path.insert(0, os.path.dirname(HERE))
    import bench
    full = json.load(open(os.path.join(os.path.dirname(HERE), "profiles", "r05_bench_full_final.json")))
    ids = "exact b128 b32 b16 b1 emu8 c2 l2 c1 mmr chat embed index rerank".split()
    for leg, i in zip(full["secondary"], ids):
        leg["id"] = i
    assert len(json.dumps(full)) > 20000
    text = json.dumps(bench.compact_line(full), allow_nan=False)
    assert len(text.encode()) <= bench.LINE_BUDGET <= 8192 and "\n" not in text
    o = _strict(text)
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data"):
        assert k in o, k
    assert o["config"]["workload"].startswith("10000000x384")
    r = o["roofline"]
    assert r["bound"] in ("hbm", "mfma") and abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-3 and r["unit"] in ("GB/s", "TFLOP/s") and "traffic" in r
    assert r["north_star"]["batch"] in (16, 32) and r["emulated_shard_8"]["emulated"] is True
    c = o["cpu_baseline"]
    assert c["value"] > 0 and c["cores"] >= 1 and c["kind"] in ("port", "reference") and c["sample"]
    assert [s["id"] for s in o["secondary"]] == ids
    for s in o["secondary"]:
        assert len(s["id"]) <= 40 and s["value"] > 0 and s["roofline"]["frac"] > 0
    # a pathological record (huge strings, 60 legs) still fits: detail is dropped in steps
    fat = dict(full, secondary=[dict(full["secondary"][i % 14], id=f"leg{i}", note="x" * 5000) for i in range(60)])
    assert len(json.dumps(bench.compact_line(fat), allow_nan=False).encode()) <= bench.LINE_BUDGET
    # non-finite values never reach the line
    assert bench._denan({"a": float("nan"), "b": [float("inf"), 1.0]}) == {"a": None, "b": [None, 1.0]}


def test_stdout_guard_sends_stray_output_to_stderr():
    code = ("import os, sys, ctypes; sys.path.insert(0, %r); import bench; g = bench._StdoutGuard(); "
            "print('stray python print'); os.write(1, b'stray fd write\\n'); ctypes.CDLL(None).puts(b'stray C puts'); g.emit('{\"ok\": 1}')") % os.path.dirname(HERE)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout == '{"ok": 1}\n', r.stdout
    assert "stray python print" in r.stderr and "stray fd write" in r.stderr and "stray C puts" in r.stderr


def test_dump_outputs_writes_the_last_timed_step(tmp_path):
    """--dump-outputs DIR: the merged top-k of the last timed step as float32 scores / float64 ids; the same arguments give the
    same inputs, so two runs dump the same arrays -- a plain run and a --full run alike (what --full adds runs after the dump)."""
    import numpy as np
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    dumps = []
    for run, full in (("a", False), ("b", True)):
        d = tmp_path / run
        r = subprocess.run([sys.executable, DRIVER, *ARGS, "--dump-outputs", str(d)] + (["--full"] if full else []),
                           capture_output=True, text=True, timeout=600, env=env)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
        o = _line(r.stdout)
        _check(o, full)
        assert o["dumped_outputs"] == {"dir": str(d), "arrays": {"scores": [16, 10], "ids": [16, 10]}}
        assert sorted(os.listdir(d)) == ["ids.npy", "scores.npy"]
        s, i = np.load(d / "scores.npy"), np.load(d / "ids.npy")
        assert s.dtype == np.float32 and i.dtype == np.float64 and s.shape == i.shape == (16, 10)
        assert (s[:, :-1] >= s[:, 1:]).all() and (i >= 0).all() and (i < 6001).all() and (i == np.rint(i)).all()
        dumps.append((s, i))
    assert np.array_equal(dumps[0][0], dumps[1][0]) and np.array_equal(dumps[0][1], dumps[1][1])


def test_dump_outputs_samples_above_the_budget(tmp_path):
    sys.path.insert(0, os.path.dirname(HERE))
    import numpy as np
    import torch
    import bench
    s = torch.arange(1000 * 10, dtype=torch.float32).reshape(1000, 10)
    r = torch.arange(1000 * 10, dtype=torch.int64).reshape(1000, 10)
    shapes = bench.dump_outputs(str(tmp_path / "a"), s, r, budget=100 * 128)
    assert shapes == {"scores": [97, 10], "ids": [97, 10], "query_rows": [97]}
    rows = np.load(tmp_path / "a" / "query_rows.npy")
    assert sum(os.path.getsize(tmp_path / "a" / f"{n}.npy") for n in shapes) <= 100 * 128     # headers included
    assert np.array_equal(np.load(tmp_path / "a" / "ids.npy"), r.numpy()[rows.astype(np.int64)].astype(np.float64))
    bench.dump_outputs(str(tmp_path / "b"), s, r, budget=100 * 128)    # the sample is fixed
    assert np.array_equal(rows, np.load(tmp_path / "b" / "query_rows.npy"))
    assert bench.dump_outputs(str(tmp_path / "c"), s, r) == {"scores": [1000, 10], "ids": [1000, 10]}
