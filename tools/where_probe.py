"""Filtered search through device fields against the host route it stands beside, in ONE process: two MI355XVectorStore objects over the
same records and vectors, one with device_fields=("source",) -- conditions resolved on the device (rmu_index_search_where) -- and one
without, which is the route the store always had (field maps in Python, int64 row lists uploaded per call), unchanged code.

  (a) the first filtered query after an add_texts of 1 000 records (the reference uploads between /chat requests): the host route walks
      every record to rebuild its field map, the device route encodes the 1 000 new records during the add and uploads their codes;
  (b) steady state: one batch call with 1, 8 and 128 distinct conditions (one query each) at 0.1 %, 1 % and 10 % selectivity;
  (c) the selection alone (Columns.select with a device output): kernel times of count + scan and of the write pass from events
      (RMU_COLUMNS_TIMING, which this script sets together with RMU_TUNING), and their bytes against the 8 TB/s roof.

A condition is `source in [values]` over 1 000 equally frequent values: 1, 10 and 100 values give the three selectivities, different
conditions take different values.  The legs of (b) alternate (host, device, host again); the two host legs give the run-to-run spread
((max - min) / min over all their windows) the device leg is held against.  A window is enough calls to fill --window seconds; medians
with [min, max] over --reps windows.  Both stores return the same documents and scores for every shape before anything is timed.

  python tools/where_probe.py [--rows 1000000] [--dim 384] [--k 10] [--window 0.2] [--reps 5] [--commit ID] [--out profiles/where_search.md]

Writes the tables between the two marker lines of --out (everything else in that file is kept) and prints one JSON line."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time
import zlib

os.environ.setdefault("RMU_TUNING", "1")
os.environ.setdefault("RMU_COLUMNS_TIMING", "1")

import numpy as np  # noqa: E402
import torch  # noqa: E402

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ragmeup_amd import _native as N  # noqa: E402
from ragmeup_amd.vectorstore import MI355XVectorStore  # noqa: E402

HBM_BYTES_PER_S = 8e12
BEGIN, END = "<!-- measured: begin (tools/where_probe.py) -->", "<!-- measured: end -->"
N_VALUES = 1000


class SyntheticEmbeddings:
    """Unit vectors: documents from a seeded device generator (the same sequence for two objects made alike), queries from their text."""

    def __init__(self, dim):
        self.dim, self.calls = dim, 0

    def embed_documents_device(self, texts):
        g = torch.Generator(device="cuda")
        g.manual_seed(1000 + self.calls)
        self.calls += 1
        x = torch.randn((len(texts), self.dim), generator=g, dtype=torch.float32, device="cuda")
        return x / x.norm(dim=1, keepdim=True)

    def embed_documents_array(self, texts):
        out = np.stack([np.random.default_rng(zlib.crc32(t.encode())).standard_normal(self.dim) for t in texts]).astype(np.float32)
        return out / np.linalg.norm(out, axis=1, keepdims=True)

    def embed_documents(self, texts):
        return self.embed_documents_array(texts).tolist()

    def embed_query(self, text):
        return self.embed_documents_array([text])[0].tolist()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=384)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--conditions", default="1,8,128")
    ap.add_argument("--fractions", default="0.001,0.01,0.1")
    ap.add_argument("--window", type=float, default=0.2, help="seconds of work per timed window")
    ap.add_argument("--reps", type=int, default=5, help="windows per leg (at least 5)")
    ap.add_argument("--commit", default="unknown", help="the commit the numbers belong to (written into the file)")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "where_search.md"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("where_probe: no GPU: there is nothing to measure without one")
    torch.cuda.set_device(0)
    rng = np.random.default_rng(7)
    value = lambda v: "file%04d.pdf" % v

    def records(lo, hi, vals):
        return (["chunk %d" % i for i in range(lo, hi)], [{"source": value(int(v)), "page": i % 7} for i, v in zip(range(lo, hi), vals)],
                ["pk%08d" % i for i in range(lo, hi)])

    t0 = time.perf_counter()
    vals = rng.integers(0, N_VALUES, a.rows)
    stores = {}
    for name, kw in (("host", {}), ("device", {"device_fields": ("source",)})):
        st = MI355XVectorStore(embeddings=SyntheticEmbeddings(a.dim), collection_name="where-probe-" + name, auto_persist=False, device=0,
                               pipeline_inserts=False, **kw)
        st.add_texts(*records(0, a.rows, vals))
        st.flush()
        stores[name] = st
    host, dev = stores["host"], stores["device"]
    assert hasattr(dev._index, "search_where") and len(dev._columns) == len(dev._index) == a.rows
    setup_s = time.perf_counter() - t0
    print(json.dumps({"setup_s": round(setup_s, 1)}), file=sys.stderr, flush=True)

    def summary(v):
        return {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}

    def same(x, y):
        return [[(d.page_content, d.metadata, s) for d, s in g] for g in x] == [[(d.page_content, d.metadata, s) for d, s in g] for g in y]

    # ---- (a) the first filtered query after an upload of 1 000 records ----------------------------------------------------------------
    qv = SyntheticEmbeddings(a.dim).embed_query("what does the first file say")
    first = {"host": [], "device": []}
    add_ms = {"host": [], "device": []}
    n_now = a.rows
    builds0 = dev._field_map_builds
    for rep in range(a.reps):
        new_vals = rng.integers(0, N_VALUES, 1000)
        got = {}
        for name, st in stores.items():
            t1 = time.perf_counter()
            st.add_texts(*records(n_now, n_now + 1000, new_vals))
            add_ms[name].append((time.perf_counter() - t1) * 1e3)
            t1 = time.perf_counter()
            got[name] = st.similarity_search_with_score_by_vector(qv, a.k, filter={"source": value(7 + rep)})
            first[name].append((time.perf_counter() - t1) * 1e3)
        assert same([got["host"]], [got["device"]])
        n_now += 1000
    assert dev._field_map_builds == builds0
    case_a = {"rows": n_now, "first_query_host": summary(first["host"]), "first_query_device": summary(first["device"]),
              "add_texts_1000_host": summary(add_ms["host"]), "add_texts_1000_device": summary(add_ms["device"])}
    print(json.dumps(case_a), file=sys.stderr, flush=True)

    # ---- (b) steady state ----------------------------------------------------------------------------------------------------------------
    def window(fn, calls):
        t1 = time.perf_counter()
        for _ in range(calls):
            fn()
        return (time.perf_counter() - t1) * 1e3 / calls

    def calls_for(fn):
        fn()                                                      # warm-up of this shape (the host route builds its map here)
        ms = window(fn, 1)
        return max(1, int(a.window * 1e3 / max(ms, 1e-3)))

    case_b = []
    for f in (float(v) for v in a.fractions.split(",")):
        per = max(1, int(round(f * N_VALUES)))
        for nc in (int(v) for v in a.conditions.split(",")):
            filters = [{"source": [value(int(v)) for v in rng.choice(N_VALUES, per, replace=False)]} for _ in range(nc)]
            queries = ["request %d of shape %d %g" % (i, nc, f) for i in range(nc)]
            emb = np.asarray(SyntheticEmbeddings(a.dim).embed_documents_array(queries))
            for st in stores.values():                            # the query embedding is not what is measured: both stores look it up
                st._embeddings.embed_documents_array = lambda texts, emb=emb: emb
            run = {name: (lambda st=st: st.similarity_search_with_score_batch(queries, a.k, filters=filters)) for name, st in stores.items()}
            assert same(run["host"](), run["device"]())
            n_h, n_d = calls_for(run["host"]), calls_for(run["device"])
            t_a, t_d, t_b = [], [], []
            for _ in range(a.reps):
                t_a.append(window(run["host"], n_h))
                t_d.append(window(run["device"], n_d))
                t_b.append(window(run["host"], n_h))
            med_a, med_d, med_b = (statistics.median(v) for v in (t_a, t_d, t_b))
            spread = (max(t_a + t_b) - min(t_a + t_b)) / min(t_a + t_b)
            best_h = min(med_a, med_b)
            verdict = "device" if med_d < best_h * (1.0 - spread) else "host" if med_d > max(med_a, med_b) * (1.0 + spread) else "undecided"
            case_b.append({"fraction": f, "rows_per_condition": int(round(f * n_now)), "conditions": nc, "host": summary(t_a), "device": summary(t_d),
                           "host_again": summary(t_b), "calls_per_window": [n_h, n_d], "run_to_run_spread": round(spread, 4),
                           "device_over_host": round(med_d / best_h, 4), "ahead_by_more_than_the_spread": verdict})
            print(json.dumps(case_b[-1]), file=sys.stderr, flush=True)
    for st in stores.values():
        del st._embeddings.embed_documents_array

    # ---- (c) the selection alone -----------------------------------------------------------------------------------------------------------
    lib = N.lib()
    cols, codes = dev._columns, dev._dev_codes[0]
    case_c = []
    for f in (float(v) for v in a.fractions.split(",")):
        per = max(1, int(round(f * N_VALUES)))
        for nc in (int(v) for v in a.conditions.split(",")):
            sels = [[(0, [codes[value(int(v))] for v in rng.choice(N_VALUES, per, replace=False)])] for _ in range(nc)]
            cnt, wr, wall, rows_out = [], [], [], 0
            for _ in range(2 + max(5, a.reps)):
                t1 = time.perf_counter()
                lists = cols.select(sels, device=True)
                wall.append((time.perf_counter() - t1) * 1e3)
                c_ms, w_ms = ctypes.c_float(), ctypes.c_float()
                lib.rmu_columns_last_ms_(ctypes.byref(c_ms), ctypes.byref(w_ms))
                cnt.append(c_ms.value); wr.append(w_ms.value)
                rows_out = sum(int(x.shape[0]) for x in lists)
            cnt, wr, wall = cnt[2:], wr[2:], wall[2:]
            b_count = nc * n_now * 4                               # one field, read once per selection
            b_write = nc * n_now * 4 + rows_out * 8
            case_c.append({"fraction": f, "selections": nc, "rows_out": rows_out, "count_scan_ms": summary(cnt), "write_ms": summary(wr),
                           "select_call_wall_ms": summary(wall), "count_bytes": b_count, "write_bytes": b_write,
                           "count_roofline_fraction": round(b_count / (statistics.median(cnt) * 1e-3) / HBM_BYTES_PER_S, 4),
                           "write_roofline_fraction": round(b_write / (statistics.median(wr) * 1e-3) / HBM_BYTES_PER_S, 4)})
            print(json.dumps(case_c[-1]), file=sys.stderr, flush=True)

    head = {"probe": "where_search", "commit": a.commit, "rows": a.rows, "dim": a.dim, "k": a.k, "window_s": a.window, "reps": a.reps,
            "device": torch.cuda.get_device_name(0), "hip": getattr(torch.version, "hip", None), "setup_s": round(setup_s, 1)}
    print(json.dumps({**head, "first_query_after_add": case_a, "steady_state": case_b, "selection": case_c}), flush=True)

    fmt = lambda s: f"{s['median_ms']:.4f} [{s['min_ms']:.4f}, {s['max_ms']:.4f}]"
    out = [BEGIN, f"Commit {a.commit}; {head['device']} (HIP {head['hip']}); {a.rows} x {a.dim} fp32 rows (unit-norm synthetic), k = {a.k}, `source` holds "
           f"{N_VALUES} equally frequent values; windows of {a.window} s, {a.reps} windows per leg; medians [min, max] of the wall time per call in ms.", "",
           f"**(a) first filtered query after an `add_texts` of 1 000 records** ({a.reps} uploads, {case_a['rows']} rows at the end)", "",
           "| store | first filtered query ms | the add_texts call in front of it ms |", "|---|---|---|",
           f"| without device_fields (host route) | {fmt(case_a['first_query_host'])} | {fmt(case_a['add_texts_1000_host'])} |",
           f"| device_fields=(\"source\",) | {fmt(case_a['first_query_device'])} | {fmt(case_a['add_texts_1000_device'])} |", "",
           "**(b) steady state: one `similarity_search_with_score_batch(filters=...)` call, one query per distinct condition**", "",
           "| rows per condition | conditions | host route ms | device route ms | host route again ms | spread | device / host | ahead by more than the spread |",
           "|---|---|---|---|---|---|---|---|"]
    for r in case_b:
        out.append(f"| {r['rows_per_condition']} ({100 * r['fraction']:g} %) | {r['conditions']} | {fmt(r['host'])} | {fmt(r['device'])} | {fmt(r['host_again'])} | "
                   f"{100 * r['run_to_run_spread']:.1f} % | {r['device_over_host']:.3f} | {r['ahead_by_more_than_the_spread']} |")
    out += ["", "**(c) the selection alone: `Columns.select`, device output** (kernel times from events; bytes = 4 per row and selection read by each pass, "
            "+ 8 per selected row written)", "",
            "| selectivity | selections | rows out | count + scan ms | share of 8 TB/s | write ms | share of 8 TB/s | whole call, wall ms |", "|---|---|---|---|---|---|---|---|"]
    for r in case_c:
        out.append(f"| {100 * r['fraction']:g} % | {r['selections']} | {r['rows_out']} | {fmt(r['count_scan_ms'])} | {r['count_roofline_fraction']:.3f} | "
                   f"{fmt(r['write_ms'])} | {r['write_roofline_fraction']:.3f} | {fmt(r['select_call_wall_ms'])} |")
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
