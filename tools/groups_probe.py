"""Grouped filtered search against the per-list calls it replaces, in ONE process on ONE index: for every shape (number of lists x list
length x queries per list) the wall time of one FlatIndex.search_groups call next to that of the loop of FlatIndex.search(rows=list)
calls over the same lists and queries -- host arrays in, host arrays out on both sides, which is how MI355XVectorStore calls them.  The
yardstick is the per-list path, whose code the grouped form does not touch.  The legs alternate (per-list, grouped, per-list again); the
two per-list legs give the run-to-run spread ((max - min) / min over all their windows) the grouped leg has to beat.  A window is enough calls to fill `--window` seconds; every
shape is warmed up; medians with [min, max] over `--reps` windows.  The scan launches of the grouped call are timed apart
(rmu_set_timing: a pair of events around them) for their share of the 8 TB/s roofline on the bytes they gather.

  python tools/groups_probe.py [--rows 1000000] [--dim 384] [--k 10] [--lists 1,2,8,32,128] [--fractions 0.001,0.01,0.1] [--per-list 1,4]
                               [--window 0.25] [--reps 5] [--out profiles/groups_search.md]

Writes the table between the two marker lines of --out (everything else in that file is kept) and prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ragmeup_amd import FlatIndex  # noqa: E402

HBM_BYTES_PER_S = 8e12
BEGIN, END = "<!-- measured: begin (tools/groups_probe.py) -->", "<!-- measured: end -->"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=384)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--lists", default="1,2,8,32,128")
    ap.add_argument("--fractions", default="0.001,0.01,0.1")
    ap.add_argument("--per-list", default="1,4", help="queries per list")
    ap.add_argument("--window", type=float, default=0.25, help="seconds of work per timed window")
    ap.add_argument("--reps", type=int, default=5, help="windows per leg")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "groups_search.md"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("groups_probe: no GPU: there is nothing to measure without one")
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
    torch.cuda.synchronize()
    rng = np.random.default_rng(99)
    n_lists = [int(v) for v in a.lists.split(",")]
    fractions = [float(v) for v in a.fractions.split(",")]
    per_list = [int(v) for v in getattr(a, "per_list").split(",")]

    def window(fn, calls):
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        return (time.perf_counter() - t0) * 1e3 / calls          # ms per call (every call drains its stream: wall time is call time)

    def calls_for(fn):
        window(fn, 2)                                             # warm-up of this shape
        ms = window(fn, 3)
        return max(3, int(a.window * 1e3 / max(ms, 1e-3)))

    def summary(v):
        return {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}

    results = []
    for f in fractions:
        m = max(1, int(round(f * a.rows)))
        for nl in n_lists:
            lists = [np.sort(rng.choice(a.rows, m, replace=False)).astype(np.int64) for _ in range(nl)]
            for per in per_list:
                nq = nl * per
                q = rng.standard_normal((nq, a.dim)).astype(np.float32)
                q /= np.linalg.norm(q, axis=1, keepdims=True)
                q_list = np.repeat(np.arange(nl), per)
                blocks = [np.ascontiguousarray(q[i * per:(i + 1) * per]) for i in range(nl)]

                def loop():
                    return [idx.search(blocks[i], a.k, rows=lists[i]) for i in range(nl)]

                def grouped():
                    return idx.search_groups(q, a.k, lists, q_list)

                ref, got = loop(), grouped()                       # the two legs answer alike, bit for bit
                assert all(np.array_equal(got[1][i * per:(i + 1) * per], ref[i][1]) and
                           np.array_equal(got[0][i * per:(i + 1) * per].view(np.int32), ref[i][0].view(np.int32)) for i in range(nl))
                n_loop, n_grp = calls_for(loop), calls_for(grouped)
                t_a, t_g, t_b = [], [], []
                for _ in range(a.reps):                            # alternate: per-list, grouped, per-list again
                    t_a.append(window(loop, n_loop))
                    t_g.append(window(grouped, n_grp))
                    t_b.append(window(loop, n_loop))
                idx.set_timing(True)
                scan = []
                for _ in range(9):
                    grouped()
                    scan.append(idx.last_scan_ms())
                launches = idx.last_geometry()["launches"]
                idx.set_timing(False)
                nbytes = nl * m * dpad * 4                         # (at most 32 queries per list here: every row is gathered once)
                med_a, med_g, med_b = (statistics.median(v) for v in (t_a, t_g, t_b))
                spread = (max(t_a + t_b) - min(t_a + t_b)) / min(t_a + t_b)      # every window of the two per-list legs
                results.append({"fraction": f, "list_rows": m, "lists": nl, "queries_per_list": per, "per_list": summary(t_a), "grouped": summary(t_g),
                                "per_list_again": summary(t_b), "calls_per_window": [n_loop, n_grp], "run_to_run_spread": round(spread, 4),
                                "grouped_over_per_list": round(med_g / min(med_a, med_b), 4),
                                "grouped_is_faster_by_more_than_the_spread": bool(med_g < min(med_a, med_b) * (1.0 - spread)),
                                "scan_launches": launches, "scan_ms": round(statistics.median(scan), 4), "gathered_bytes": nbytes,
                                "scan_roofline_fraction": round(nbytes / (statistics.median(scan) * 1e-3) / HBM_BYTES_PER_S, 4)})
                print(json.dumps(results[-1]), file=sys.stderr, flush=True)
    head = {"probe": "groups_search", "rows": a.rows, "dim": a.dim, "k": a.k, "window_s": a.window, "reps": a.reps, "device": torch.cuda.get_device_name(0)}
    print(json.dumps({**head, "results": results}), flush=True)

    fmt = lambda s: f"{s['median_ms']:.4f} [{s['min_ms']:.4f}, {s['max_ms']:.4f}]"
    rows = ["| list rows | lists | queries per list | per-list calls ms | one grouped call ms | per-list calls again ms | spread | grouped / per-list | faster by more than the spread | scan launches | scan ms | scan share of 8 TB/s |",
            "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in results:
        rows.append(f"| {r['list_rows']} ({100 * r['fraction']:g} %) | {r['lists']} | {r['queries_per_list']} | {fmt(r['per_list'])} | {fmt(r['grouped'])} | "
                    f"{fmt(r['per_list_again'])} | {100 * r['run_to_run_spread']:.1f} % | {r['grouped_over_per_list']:.3f} | "
                    f"{'yes' if r['grouped_is_faster_by_more_than_the_spread'] else 'no'} | {r['scan_launches']} | {r['scan_ms']:.4f} | {r['scan_roofline_fraction']:.3f} |")
    table = "\n".join([BEGIN, f"{head['device']}, {a.rows} x {a.dim} fp32 rows (unit-norm synthetic), k = {a.k}, windows of {a.window} s, {a.reps} windows per leg; "
                       "medians [min, max] of the wall time per call, host arrays in and out.", ""] + rows + [END])
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
