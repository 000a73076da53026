"""Grouped search (FlatIndex.search_distinct: scan_distinct_kernel + k_distinct_fold) against the exact scan it is built from
(FlatIndex.search with screening off), in ONE process, same index, same queries.

The distinct scan reads the bytes the exact scan reads, so the expectation the numbers are held against is: parity, plus the fold, plus
the compactions' drains of the LDS-DMA ring (scan_distinct.hip).  Per (group layout, nq): wall time per call of both searches -- the legs
alternate (exact, distinct, exact again); the two exact legs give the run-to-run spread -- their ratio, the kernel times of the distinct
scan and of the fold from events (rmu_set_timing), the exact scan's kernel time the same way, and the number of part lists folded.

Group layouts: `contiguous S` -- code = row // S, the chunks of a document lie next to each other (S = 1: one row per group); `interleaved
S` -- code = row % (rows / S), the same group sizes with every group spread over the whole corpus.  A workgroup scans a contiguous row
range: with contiguous groups larger than its range / k it never meets k groups, gets no threshold and compacts at every tile.

  python tools/distinct_probe.py [--rows 1000000] [--dim 384] [--k 10] [--nq 1,32,128,1024] [--sizes 1,100,10000] [--window 0.3] [--reps 5]
                                 [--commit ID] [--out profiles/distinct_search.md]

Writes the table between the two marker lines of --out (everything else in that file is kept) and prints one JSON line."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import ragmeup_amd  # noqa: E402
from ragmeup_amd import _native as N  # noqa: E402

BEGIN, END = "<!-- measured: begin (tools/distinct_probe.py) -->", "<!-- measured: end -->"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=384)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--nq", default="1,32,128,1024")
    ap.add_argument("--sizes", default="1,100,10000")
    ap.add_argument("--window", type=float, default=0.3, help="seconds of work per timed window")
    ap.add_argument("--reps", type=int, default=5, help="windows per leg")
    ap.add_argument("--commit", default="unknown", help="the commit the numbers belong to (written into the file)")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "distinct_search.md"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("distinct_probe: no GPU: there is nothing to measure without one")
    torch.cuda.set_device(0)
    lib = N.lib()
    g = torch.Generator(device="cuda")
    g.manual_seed(11)
    idx = ragmeup_amd.FlatIndex(a.dim)
    idx.set_screening(False)
    for lo in range(0, a.rows, 250_000):
        x = torch.randn((min(250_000, a.rows - lo), a.dim), generator=g, dtype=torch.float32, device="cuda")
        idx.add(x / x.norm(dim=1, keepdim=True))
    del x
    qs = np.random.default_rng(5).standard_normal((max(int(v) for v in a.nq.split(",")), a.dim)).astype(np.float32)
    qs /= np.linalg.norm(qs, axis=1, keepdims=True)
    rows = np.arange(a.rows, dtype=np.int64)
    layouts = [("contiguous", s, rows // s) for s in (int(v) for v in a.sizes.split(","))]
    layouts += [("interleaved", s, rows % max(1, a.rows // s)) for s in (int(v) for v in a.sizes.split(",")) if s > 1]

    def summary(v):
        return {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}

    def window(fn, calls):
        t1 = time.perf_counter()
        for _ in range(calls):
            fn()
        return (time.perf_counter() - t1) * 1e3 / calls

    def calls_for(fn):
        fn()
        return max(1, int(a.window * 1e3 / max(window(fn, 1), 1e-3)))

    def kernel_ms(fn, n=5):
        """(scan ms, fold ms, parts) medians of n timed calls (events around the kernels)"""
        idx.set_timing(True)
        scan, fold, parts = [], [], 0
        for _ in range(n):
            fn()
            scan.append(idx.last_scan_ms())
            f, p = ctypes.c_float(-1.0), ctypes.c_int(0)
            lib.rmu_last_distinct_(ctypes.byref(f), ctypes.byref(p))
            fold.append(f.value); parts = p.value
        idx.set_timing(False)
        return statistics.median(scan), statistics.median(fold), parts

    results = []
    for name, size, codes in layouts:
        cols = ragmeup_amd.Columns(1)
        cols.append(np.ascontiguousarray(codes[:, None], np.int32))
        for nq in (int(v) for v in a.nq.split(",")):
            q = np.ascontiguousarray(qs[:nq])
            exact = lambda: idx.search(q, a.k)
            dist = lambda: idx.search_distinct(q, a.k, cols, 0)
            es, er = exact()
            ds, dr = dist()
            if size == 1:                                          # one row per group: the same answer, bit for bit
                assert np.array_equal(er, dr) and np.array_equal(es.view(np.uint32), ds.view(np.uint32))
            else:                                                  # one row per group in the answer, the best row first
                assert all(len(set(codes[r[r >= 0]].tolist())) == int((r >= 0).sum()) for r in dr) and np.array_equal(er[:, 0], dr[:, 0])
            n_e, n_d = calls_for(exact), calls_for(dist)
            t_a, t_d, t_b = [], [], []
            for _ in range(a.reps):
                t_a.append(window(exact, n_e))
                t_d.append(window(dist, n_d))
                t_b.append(window(exact, n_e))
            e_scan, _, _ = kernel_ms(exact)
            d_scan, d_fold, parts = kernel_ms(dist)
            both = t_a + t_b
            res = {"layout": name, "group_rows": size, "nq": nq, "exact": summary(both), "distinct": summary(t_d),
                   "run_to_run_spread": round((max(both) - min(both)) / min(both), 4),
                   "distinct_over_exact": round(statistics.median(t_d) / statistics.median(both), 4),
                   "exact_scan_kernel_ms": round(e_scan, 4), "distinct_scan_kernel_ms": round(d_scan, 4), "fold_kernel_ms": round(d_fold, 4), "parts": parts,
                   "calls_per_window": [n_e, n_d]}
            results.append(res)
            print(json.dumps(res), file=sys.stderr, flush=True)
        cols.close()

    head = {"probe": "distinct_search", "commit": a.commit, "rows": a.rows, "dim": a.dim, "k": a.k, "window_s": a.window, "reps": a.reps,
            "device": torch.cuda.get_device_name(0), "hip": getattr(torch.version, "hip", None)}
    print(json.dumps({**head, "results": results}), flush=True)

    fmt = lambda s: f"{s['median_ms']:.4f} [{s['min_ms']:.4f}, {s['max_ms']:.4f}]"
    out = [BEGIN, f"Commit {a.commit}; {head['device']} (HIP {head['hip']}); {a.rows} x {a.dim} fp32 unit rows, k = {a.k}, host queries and results; "
           f"windows of {a.window} s, {a.reps} windows per leg (exact: two legs around the distinct one); wall ms per call as median [min, max]; kernel ms: "
           "medians of 5 calls between events.", "",
           "| groups | nq | exact search ms | distinct search ms | spread of exact | distinct / exact | exact scan kernel ms | distinct scan kernel ms | fold kernel ms | parts |",
           "|---|---|---|---|---|---|---|---|---|---|"]
    for r in results:
        out.append(f"| {r['layout']} {r['group_rows']} | {r['nq']} | {fmt(r['exact'])} | {fmt(r['distinct'])} | {100 * r['run_to_run_spread']:.1f} % | "
                   f"{r['distinct_over_exact']:.3f} | {r['exact_scan_kernel_ms']:.4f} | {r['distinct_scan_kernel_ms']:.4f} | {r['fold_kernel_ms']:.4f} | {r['parts']} |")
    out.append(END)
    table = "\n".join(out)
    old = open(a.out).read() if os.path.exists(a.out) else ""
    if BEGIN in old and END in old:
        new = old[:old.index(BEGIN)] + table + old[old.index(END) + len(END):]
    else:
        new = old + ("\n" if old and not old.endswith("\n") else "") + table + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(new)


if __name__ == "__main__":
    main()
