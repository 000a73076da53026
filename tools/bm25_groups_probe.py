"""Grouped filtered BM25 search against the per-list calls it replaces, in ONE process on ONE index (the method of tools/groups_probe.py):
for every shape (number of lists x documents per list x queries per list, once with lists that are contiguous runs of ids -- an upload --
and once with random ascending ids) the wall time of one BM25Index.search_groups call next to that of the loop of
BM25Index.search(docs=list) calls over the same lists and queries.  The yardstick is the per-list path, whose code the grouped form does
not touch.  The legs alternate (per-list, grouped, per-list again); the two per-list legs give the run-to-run spread ((max - min) / min
over all their windows) the grouped leg has to beat.  A window is enough calls to fill `--window` seconds; every shape is warmed up; medians
with [min, max] over `--reps` windows.  Before anything is timed the two legs must return the same bits.  Per shape the table also says how
many tiles the plan keeps of all the tiles its queries would otherwise walk, and how many bytes of mask it uploads (from the library's own
planner, rmu_bm25_groups_plan_, at the geometry the call chooses: bm25.hip, "geometry").

  python tools/bm25_groups_probe.py [--docs 1000000] [--vocab 50000] [--k 4] [--lists 1,2,8,32,128] [--list-docs 1000,10000,100000]
                                    [--per-list 1,4] [--window 0.25] [--reps 5] [--out profiles/bm25_groups.md]

Corpus and queries are tools/bm25_probe.py's.  Writes the table between the two marker lines of --out (everything else in that file is
kept) and prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bm25_probe import corpus, queries  # noqa: E402

BEGIN, END = "<!-- measured: begin (tools/bm25_groups_probe.py) -->", "<!-- measured: end -->"


def geometry(ids_of_queries: int, nq: int):
    """the tile and the part cap rmu_bm25_search_groups chooses with no option set (bm25.hip: pick_tile, pick_max_wgs)"""
    tile = 8192
    while tile > 1024 and ids_of_queries // tile + nq < 1024:
        tile >>= 1
    return tile, min(1024, max(8, 4096 // nq))


def plan_counts(lib, n_docs, live, lists, q_list):
    """(kept tiles summed over the queries, tiles of the corpus x queries, mask bytes uploaded)"""
    ptr = np.zeros(len(lists) + 1, np.int64)
    np.cumsum([x.size for x in lists], out=ptr[1:])
    docs = np.ascontiguousarray(np.concatenate(lists))
    ql = np.ascontiguousarray(q_list, dtype=np.int32)
    tile, cap = geometry(int(sum(lists[g].size for g in q_list)), ql.size)
    counts = np.zeros(4, np.int64)
    rc = lib.rmu_bm25_groups_plan_(n_docs, live.ctypes.data, tile, cap, docs.ctypes.data, ptr.ctypes.data, len(lists), ql.ctypes.data, ql.size,
                                   None, 0, None, 0, counts.ctypes.data)
    assert rc == 0
    per_list = np.bincount(ql, minlength=len(lists))
    kept = 0
    for g, x in enumerate(lists):
        kept += int(np.unique(x // tile).size) * int(per_list[g])
    return kept, -(-n_docs // tile) * int(ql.size), int(counts[1]) * 4, tile


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1_000_000)
    ap.add_argument("--vocab", type=int, default=50_000)
    ap.add_argument("--k", type=int, default=4)
    ap.add_argument("--lists", default="1,2,8,32,128")
    ap.add_argument("--list-docs", default="1000,10000,100000")
    ap.add_argument("--per-list", default="1,4", help="queries per list")
    ap.add_argument("--window", type=float, default=0.25, help="seconds of work per timed window")
    ap.add_argument("--reps", type=int, default=5, help="windows per leg")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bm25_groups.md"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bm25_groups_probe: no GPU: there is nothing to measure without one")
    from ragmeup_amd import _native
    from ragmeup_amd.bm25 import BM25Index
    lib = _native.lib()
    texts = corpus(a.docs, a.vocab)
    ix = BM25Index()
    ix.add_texts(texts)
    pool = queries(texts, 512)
    ix.search(pool[:1], a.k)                                          # the image upload is not part of any leg
    live = np.ones(a.docs, np.uint8)
    rng = np.random.default_rng(99)
    n_lists = [int(v) for v in a.lists.split(",")]
    list_docs = [int(v) for v in getattr(a, "list_docs").split(",")]
    per_list = [int(v) for v in getattr(a, "per_list").split(",")]

    def window(fn, calls):
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        return (time.perf_counter() - t0) * 1e3 / calls              # ms per call (every call drains its stream: wall time is call time)

    def calls_for(fn):
        window(fn, 2)                                                 # warm-up of this shape
        ms = window(fn, 3)
        return max(3, int(a.window * 1e3 / max(ms, 1e-3)))

    def summary(v):
        return {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}

    results = []
    for m in list_docs:
        for nl in n_lists:
            for kind in ("contiguous", "random"):
                if kind == "contiguous":                              # an upload: a run of consecutive ids, anywhere in the corpus
                    starts = rng.integers(0, a.docs - m + 1, nl)
                    lists = [np.arange(s, s + m, dtype=np.int64) for s in starts]
                else:
                    lists = [np.sort(rng.choice(a.docs, m, replace=False)).astype(np.int64) for _ in range(nl)]
                for per in per_list:
                    nq = nl * per
                    qs = [pool[int(i)] for i in rng.integers(0, len(pool), nq)]
                    q_list = np.repeat(np.arange(nl), per)
                    blocks = [qs[i * per:(i + 1) * per] for i in range(nl)]

                    def loop():
                        return [ix.search(blocks[i], a.k, docs=lists[i]) for i in range(nl)]

                    def grouped():
                        return ix.search_groups(qs, a.k, lists, q_list)

                    ref, got = loop(), grouped()                       # bits first: the two legs answer alike
                    assert all(np.array_equal(got[1][i * per:(i + 1) * per], ref[i][1]) and
                               np.array_equal(got[0][i * per:(i + 1) * per].view(np.int32), ref[i][0].view(np.int32)) for i in range(nl)), (m, nl, kind, per)
                    n_loop, n_grp = calls_for(loop), calls_for(grouped)
                    t_a, t_g, t_b = [], [], []
                    for _ in range(a.reps):                            # alternate: per-list, grouped, per-list again
                        t_a.append(window(loop, n_loop))
                        t_g.append(window(grouped, n_grp))
                        t_b.append(window(loop, n_loop))
                    med_a, med_g, med_b = (statistics.median(v) for v in (t_a, t_g, t_b))
                    spread = (max(t_a + t_b) - min(t_a + t_b)) / min(t_a + t_b)      # every window of the two per-list legs
                    kept, tiles, mask_bytes, tile = plan_counts(lib, a.docs, live, lists, q_list)
                    results.append({"list_docs": m, "lists": nl, "kind": kind, "queries_per_list": per, "per_list": summary(t_a),
                                    "grouped": summary(t_g), "per_list_again": summary(t_b), "calls_per_window": [n_loop, n_grp],
                                    "run_to_run_spread": round(spread, 4), "grouped_over_per_list": round(med_g / min(med_a, med_b), 4),
                                    "grouped_is_faster_by_more_than_the_spread": bool(med_g < min(med_a, med_b) * (1.0 - spread)),
                                    "tile": tile, "kept_tiles": kept, "all_tiles": tiles, "mask_bytes": mask_bytes,
                                    "per_list_bitmap_bytes": nl * ((a.docs + 31) // 32 + 1) * 4})
                    print(json.dumps(results[-1]), file=sys.stderr, flush=True)
    head = {"probe": "bm25_groups", "docs": a.docs, "vocab": a.vocab, "k": a.k, "query_tokens": [8, 16], "window_s": a.window, "reps": a.reps,
            "device": torch.cuda.get_device_name(0)}
    print(json.dumps({**head, "results": results}), flush=True)

    fmt = lambda s: f"{s['median_ms']:.4f} [{s['min_ms']:.4f}, {s['max_ms']:.4f}]"
    rows = ["| list docs | lists | ids | queries per list | per-list calls ms | one grouped call ms | per-list calls again ms | spread | grouped / per-list | "
            "faster by more than the spread | tile | kept tiles / all tiles | mask bytes (grouped) | bitmap bytes (per-list) |",
            "|---|---|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in results:
        rows.append(f"| {r['list_docs']} | {r['lists']} | {r['kind']} | {r['queries_per_list']} | {fmt(r['per_list'])} | {fmt(r['grouped'])} | "
                    f"{fmt(r['per_list_again'])} | {100 * r['run_to_run_spread']:.1f} % | {r['grouped_over_per_list']:.3f} | "
                    f"{'yes' if r['grouped_is_faster_by_more_than_the_spread'] else 'no'} | {r['tile']} | {r['kept_tiles']} / {r['all_tiles']} | "
                    f"{r['mask_bytes']} | {r['per_list_bitmap_bytes']} |")
    table = "\n".join([BEGIN, f"{head['device']}, {a.docs} documents (vocabulary {a.vocab}, Zipf-like, 0..60 words), queries of 8-16 tokens, k = {a.k}, "
                       f"windows of {a.window} s, {a.reps} windows per leg; medians [min, max] of the wall time per call, host arrays in and out.", ""]
                      + rows + [END])
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
