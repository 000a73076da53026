"""Cost of rmu_index_compact on a large index, and what it buys back.

For each dead fraction and storage path: build an N x 384 IP index from device rows, tombstone that fraction at random, time a
batch-1024 search, compact(), time the search again.  Beside it: a device-to-device copy (torch copy_, i.e. hipMemcpyAsync) of the bytes
the gather must move (read + write of every live row past the first dead one: fp32 row + fp16 image), timed with device events, as the
yardstick of the gather kernel; and the search on a freshly built index of the live row count.  Kernel-only time of k_compact_rows: run
this under `rocprofv3 --kernel-trace --stats` with --no-search.

    python tools/compact_probe.py [--rows 10000000] [--dead 0.1 0.5] [--paths oop inplace] [--no-search] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402


def rows(n, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    x = torch.empty((n, 384), device="cuda")
    for lo in range(0, n, 1 << 20):
        hi = min(n, lo + (1 << 20))
        x[lo:hi] = torch.randn((hi - lo, 384), device="cuda", generator=g)
        x[lo:hi] /= x[lo:hi].norm(dim=1, keepdim=True)
    return x


def time_search(idx, q, reps=5):
    idx.search(q, 10)
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        idx.search(q, 10)
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def d2d_copy_ms(nbytes, reps=5):
    src = torch.empty(nbytes // 4, dtype=torch.float32, device="cuda")
    dst = torch.empty_like(src)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    dst.copy_(src)
    ts = []
    for _ in range(reps):
        e0.record()
        dst.copy_(src)
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    del src, dst
    torch.cuda.empty_cache()
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--dead", type=float, nargs="+", default=[0.1, 0.5])
    ap.add_argument("--paths", nargs="+", default=["oop", "inplace"])
    ap.add_argument("--no-search", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from ragmeup_amd import FlatIndex
    n = a.rows
    x = rows(n, 1)
    q = x[torch.randint(0, n, (1024,), device="cuda")].cpu().numpy()
    q = q + 0.1 * np.random.default_rng(0).standard_normal(q.shape).astype(np.float32)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    out = []
    for frac in a.dead:
        dead = np.sort(np.random.default_rng(2).choice(n, int(frac * n), replace=False))
        first = int(dead[0])
        moved = n - dead.size - first                          # live rows past the first dead one: gathered
        gather_bytes = 2 * moved * (1536 + 768)                # read + write, fp32 row + fp16 image
        copy_ms = d2d_copy_ms(moved * (1536 + 768))
        for path in a.paths:
            idx = FlatIndex(384)
            idx.add(x)
            idx.set_compact_inplace(path == "inplace")
            idx.remove_rows(dead)
            rec = {"rows": n, "dead": frac, "path": path, "cap_before": idx.stats()["capacity"]}
            if not a.no_search:
                rec["search_ms_before"] = time_search(idx, q)
            t0 = time.perf_counter()
            idx.compact()
            rec["compact_wall_ms"] = (time.perf_counter() - t0) * 1e3
            rec["compact_ms_stat"] = idx.compaction_stats()["compact_ms"]
            rec["cap_after"] = idx.stats()["capacity"]
            rec["gather_bytes"] = gather_bytes
            rec["d2d_copy_ms"] = copy_ms
            rec["d2d_copy_GBps"] = gather_bytes / copy_ms / 1e6
            rec["compact_wall_GBps"] = gather_bytes / rec["compact_wall_ms"] / 1e6
            if not a.no_search:
                rec["search_ms_after"] = time_search(idx, q)
            idx.close()
            if not a.no_search:
                fresh = FlatIndex(384)
                fresh.add(x[: n - dead.size])
                rec["search_ms_fresh_same_rows"] = time_search(fresh, q)
                fresh.close()
            print(json.dumps(rec), flush=True)
            out.append(rec)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
