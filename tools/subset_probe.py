"""Filtered search against the exact full scan, in ONE process on ONE index: per batch size, the time of FlatIndex.search(rows=...)
(rmu_index_search_subset: the gathered scan) at several subset fractions, random and contiguous, next to the exact unfiltered scan
(set_screening(False)) of the same index, alternating the two.  Every call is enqueued on a caller stream with device queries, list and
outputs (nothing synchronises inside the window); a window is a pair of device events around enough calls to fill `--window` seconds;
every shape is warmed up; medians and the spread (min, max) over `--reps` windows.  Prints one JSON line.

  python tools/subset_probe.py [--rows 10000000] [--dim 384] [--batches 1,32] [--fractions 0.01,0.1,1.0] [--k 10] [--window 1.0] [--reps 5]

bytes of a subset search = n_sub * (dpad * 4 + 8) (the rows + the int64 list); roofline = 8 TB/s.  The time is that of the whole call
on the stream (list conversion, scan, merge, row-id mapping), not of the scan kernel alone: a kernel trace gives that."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ragmeup_amd import FlatIndex  # noqa: E402

HBM_BYTES_PER_S = 8e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=384)
    ap.add_argument("--batches", default="1,32")
    ap.add_argument("--fractions", default="0.01,0.1,1.0")
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--window", type=float, default=1.0, help="seconds of work per timed window")
    ap.add_argument("--reps", type=int, default=5, help="windows per shape (the full scan and the subset search alternate)")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("subset_probe: no GPU: there is nothing to measure without one")
    dev = torch.device("cuda", 0)
    dpad = 192 if a.dim <= 192 else 384 if a.dim <= 384 else 768
    idx = FlatIndex(a.dim, capacity_hint=a.rows, device=0)
    g = torch.Generator(device=dev)
    g.manual_seed(1234)
    for lo in range(0, a.rows, 1 << 20):
        x = torch.randn((min(a.rows, lo + (1 << 20)) - lo, a.dim), generator=g, dtype=torch.float32, device=dev)
        x /= x.norm(dim=1, keepdim=True)
        idx.add(x)
    del x
    idx.set_screening(False)                     # the unfiltered side is the exact fp32 scan
    stream = torch.cuda.Stream()
    batches = [int(v) for v in a.batches.split(",")]
    fractions = [float(v) for v in a.fractions.split(",")]
    q_all = torch.randn((max(batches), a.dim), generator=g, dtype=torch.float32, device=dev)
    q_all /= q_all.norm(dim=1, keepdim=True)
    lists = {}
    for f in fractions:
        m = max(1, min(a.rows, int(round(f * a.rows))))
        lists[(f, "random")] = (torch.arange(a.rows, device=dev) if m == a.rows
                                else torch.randperm(a.rows, generator=g, device=dev)[:m].sort().values).to(torch.int64).contiguous()
        lo = (a.rows - m) // 2
        lists[(f, "contiguous")] = torch.arange(lo, lo + m, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()

    def window(fn, calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        with torch.cuda.stream(stream):
            e0.record(stream)
            for _ in range(calls):
                fn()
            e1.record(stream)
        e1.synchronize()
        return e0.elapsed_time(e1) / calls          # ms per call

    def calls_for(fn):
        for _ in range(3):                          # warm-up of this shape
            window(fn, 2)
        ms = window(fn, 5)
        return max(5, int(a.window * 1e3 / max(ms, 1e-3)))

    def summary(v):
        return {"median_ms": round(statistics.median(v), 5), "min_ms": round(min(v), 5), "max_ms": round(max(v), 5)}

    results = []
    for b in batches:
        q = q_all[:b].contiguous()
        out = (torch.empty((b, a.k), dtype=torch.float32, device=dev), torch.empty((b, a.k), dtype=torch.int64, device=dev))
        full = lambda: idx.search(q, a.k, stream=stream.cuda_stream, out=out)
        n_full = calls_for(full)
        for (f, kind), rows in lists.items():
            sub = lambda: idx.search(q, a.k, stream=stream.cuda_stream, out=out, rows=rows)
            n_sub = calls_for(sub)
            t_full, t_sub = [], []
            for _ in range(a.reps):                 # alternate the two
                t_full.append(window(full, n_full))
                t_sub.append(window(sub, n_sub))
            nbytes = rows.numel() * (dpad * 4 + 8)
            med = statistics.median(t_sub)
            results.append({"batch": b, "fraction": f, "list": kind, "n_sub": rows.numel(), "bytes": nbytes,
                            "subset": summary(t_sub), "full_scan": summary(t_full), "calls_per_window": [n_sub, n_full],
                            "subset_over_full": round(med / statistics.median(t_full), 5),
                            "roofline_fraction_own_bytes": round(nbytes / (med * 1e-3) / HBM_BYTES_PER_S, 4)})
    line = json.dumps({"probe": "subset_search", "rows": a.rows, "dim": a.dim, "k": a.k, "window_s": a.window, "reps": a.reps,
                       "device": torch.cuda.get_device_name(0), "results": results})
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
