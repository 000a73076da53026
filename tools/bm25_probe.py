"""BM25 on the device against the reference's CPU path, one synthetic corpus: rmu_bm25_search (bm25.hip) over `--docs` documents, timed as
`--singles` single-query calls and one batch of `--batch` queries (8-16 tokens, k = 4), next to a restatement of what the reference runs per
query -- rank_bm25's get_scores (per query token a Python list comprehension over every document's term-frequency dict) + an argsort of all
N scores -- on a `--cpu-sample`-document sample of the same corpus, scaled linearly to `--docs` (labelled as sampled, as bench.py labels its
sampled baselines).  Writes one JSON line to stdout and to `--out`.

  python tools/bm25_probe.py [--docs 1000000] [--vocab 50000] [--singles 64] [--batch 64] [--k 4] [--cpu-sample 100000] [--out profiles/bm25_probe.json]

Times are host wall-clock around calls that end in a stream synchronise inside the library (the results are host arrays): they include
the query tokenisation, the descriptor copy, the scoring kernel, the merge and the copy back.  Every shape is warmed up first; the image
upload of the first search is reported separately.  "postings_bytes" is what the kernel must read for the queries: 8 bytes (document id, tf)
per posting of every query token plus the 4-byte doc_norm it gathers; bytes / time is the only rate given.
The GPU step runs in a child process under its own time limit (`--step-timeout`).

  python tools/bm25_probe.py --lifecycle [--docs 1000000] [--out profiles/bm25_lifecycle.json]

measures, on the same corpus and in one process, what removing documents costs: single-query and batch time with 0 % (bm25_topk_kernel: the
baseline) and with 10 % of the documents removed (bm25_masked_kernel); rmu_bm25_remove_docs of 1 % of the documents in one call; the first
search after that removal on the refresh path and, on a second handle with RMU_BM25_OPT_REPACK_ON_REMOVE, on the repack path; compact; save;
load + first search against building the index from the texts.  No CPU leg.
It also measures the first search after appending 1, 1000 and 100 000 documents to the `--docs` corpus, `--append-reps` times on the splice
path (RMU_BM25_OPT_REPACK_ON_ADD = 0) and as many on the repack path (= 1), alternating and starting with the repack; after every leg the
appended documents are removed and compacted away and the image is packed again, so every leg meets the same index.  The repack legs are
the yardstick: "splice_is_faster_by_more_than_the_repack_spread" is median(splice) < median(repack) - (max - min of the repack legs)."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def corpus(n, vocab, seed=0, lmax=60):
    """n documents of 0..lmax words, Zipf-like over `vocab` synthetic words"""
    rng = np.random.default_rng(seed)
    p = 1.0 / np.arange(1, vocab + 1)
    p /= p.sum()
    lens = rng.integers(0, lmax + 1, n)
    names = np.array([f"w{i}" for i in range(vocab)], dtype=object)
    words = names[rng.choice(vocab, int(lens.sum()), p=p)]
    ends = np.cumsum(lens)
    return [" ".join(words[e - l:e]) for l, e in zip(lens, ends)]


def queries(texts, n, seed=1, tmin=8, tmax=16):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        toks = []
        while len(toks) < rng.integers(tmin, tmax + 1):
            toks += texts[int(rng.integers(0, len(texts)))].split()[:3]
        out.append(" ".join(toks[:tmax]))
    return out


def summary(v):
    return {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4), "n": len(v)}


def gpu_step(a):
    from ragmeup_amd.bm25 import BM25Index
    texts = corpus(a.docs, a.vocab)
    qs = queries(texts, a.singles + a.batch)
    ix = BM25Index()
    t0 = time.perf_counter()
    for lo in range(0, len(texts), 100_000):
        ix.add_texts(texts[lo:lo + 100_000])
    add_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    ix.search(qs[:1], a.k)                                    # packs and uploads the image
    first_ms = (time.perf_counter() - t0) * 1e3

    def posting_bytes(batch):
        return sum(12 * ix.df(t) for q in batch for t in q.split())

    singles, batch = qs[:a.singles], qs[a.singles:]
    for q in singles[:5]:
        ix.search([q], a.k)
    t_single = []
    for q in singles:
        t0 = time.perf_counter()
        ix.search([q], a.k)
        t_single.append((time.perf_counter() - t0) * 1e3)
    for _ in range(3):
        ix.search(batch, a.k)
    t_batch = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        ix.search(batch, a.k)
        t_batch.append((time.perf_counter() - t0) * 1e3)
    sb, bb = posting_bytes(singles) / len(singles), posting_bytes(batch)
    res = {"stat": ix.stat(), "add_s": round(add_s, 3), "first_search_with_image_upload_ms": round(first_ms, 3),
           "single_query": dict(summary(t_single), mean_postings_bytes=int(sb),
                                postings_gb_per_s=round(sb / (statistics.median(t_single) * 1e-3) / 1e9, 2)),
           "batch": dict(summary(t_batch), queries=len(batch), postings_bytes=int(bb),
                         ms_per_query=round(statistics.median(t_batch) / len(batch), 4),
                         postings_gb_per_s=round(bb / (statistics.median(t_batch) * 1e-3) / 1e9, 2))}
    ix.close()
    print("BM25_PROBE_GPU " + json.dumps(res), flush=True)


def append_legs(a, ix, qs, batch, ms):
    """ix: every document live, image clean; it is left that way"""
    extra = corpus(100_000, a.vocab, seed=99)
    base = ix.stat()
    out = {"measured": True, "docs_before_every_leg": base["docs"], "nnz_before_every_leg": base["nnz"], "reps_per_path": a.append_reps,
           "rate": "device_bytes_moved = 16 bytes per posting of the new image (8 read from the old image or the delta, 8 written); "
                   "gb_per_s_over_the_call divides it by the whole call's median time, host work included: not a kernel rate"}
    for n in (1, 1000, 100_000):
        legs = {0: [], 1: []}
        add_ms, stats, results = [], [], []
        for rep in range(2 * a.append_reps):
            repack = 1 - rep % 2
            ix.set_option(8, repack)
            before = ix.image_stat()
            t, first = ms(lambda: ix.add_texts(extra[:n]))
            add_ms.append(t)
            t, _ = ms(lambda: ix.search(qs[:1], a.k))
            legs[repack].append(t)
            after = ix.image_stat()
            stats.append({k: after[k] - before[k] for k in after})
            assert stats[-1]["packs"] == repack and stats[-1]["splices"] == 1 - repack, stats[-1]
            results.append(ix.search(batch, a.k))
            nnz_new = ix.stat()["nnz"]
            ix.remove(np.arange(first, first + n))
            ix.compact()
            ix.search(qs[:1], a.k)                            # packs: the next leg starts from a clean image of the base corpus
            assert ix.stat()["docs"] == base["docs"] and ix.stat()["nnz"] == base["nnz"]
        same = all(np.array_equal(s.view(np.uint32), results[0][0].view(np.uint32)) and np.array_equal(d, results[0][1]) for s, d in results)
        spread = max(legs[1]) - min(legs[1])
        med0, med1 = statistics.median(legs[0]), statistics.median(legs[1])
        moved = 16 * nnz_new
        out[f"append_{n}"] = {
            "add_texts": summary(add_ms), "repack_on_add_1": dict(summary(legs[1]), spread_ms=round(spread, 4), all_ms=[round(x, 3) for x in legs[1]]),
            "repack_on_add_0_splice": dict(summary(legs[0]), all_ms=[round(x, 3) for x in legs[0]],
                                           image_stat_delta_per_leg=stats[1], device_bytes_moved=moved,
                                           gb_per_s_over_the_call=round(moved / (med0 * 1e-3) / 1e9, 2)),
            "upload_bytes_per_repack_leg": stats[0]["upload_bytes"], "results_identical_on_every_leg": bool(same),
            "splice_is_faster_by_more_than_the_repack_spread": bool(med0 < med1 - spread)}
    ix.set_option(8, 0)
    out["splice_default_holds_at_all_three_sizes"] = all(out[f"append_{n}"]["splice_is_faster_by_more_than_the_repack_spread"]
                                                         for n in (1, 1000, 100_000))
    return out


def lifecycle_step(a):
    import tempfile
    from ragmeup_amd.bm25 import BM25Index
    texts = corpus(a.docs, a.vocab)
    qs = queries(texts, a.singles + a.batch)
    singles, batch = qs[:a.singles], qs[a.singles:]
    rng = np.random.default_rng(7)
    order = rng.permutation(a.docs)
    one_pct, ten_pct = np.sort(order[:a.docs // 100]), np.sort(order[:a.docs // 10])

    def ms(fn):
        t0 = time.perf_counter()
        out = fn()
        return (time.perf_counter() - t0) * 1e3, out

    def build(repack):
        ix = BM25Index()
        ix.set_option(4, repack)
        t, _ = ms(lambda: [ix.add_texts(texts[lo:lo + 100_000]) for lo in range(0, len(texts), 100_000)])
        t2, _ = ms(lambda: ix.search(qs[:1], a.k))
        return ix, t, t2

    def timed_searches(ix):
        for q in singles[:5]:
            ix.search([q], a.k)
        t_single = [ms(lambda: ix.search([q], a.k))[0] for q in singles]
        for _ in range(3):
            ix.search(batch, a.k)
        t_batch = [ms(lambda: ix.search(batch, a.k))[0] for _ in range(a.reps)]
        return {"single_query": summary(t_single), "batch": dict(summary(t_batch), queries=len(batch))}

    ix, add_ms, first_ms = build(0)
    res = {"stat": ix.stat(), "build_from_texts": {"add_texts_ms": round(add_ms, 1), "first_search_with_image_upload_ms": round(first_ms, 1)}}
    res["removed_0pct_plain_kernel"] = timed_searches(ix)
    res["first_search_after_append"] = append_legs(a, ix, qs, batch, ms)
    t, n = ms(lambda: ix.remove(one_pct))
    res["remove_1pct_one_call"] = {"ms": round(t, 2), "documents": n}
    t, _ = ms(lambda: ix.search(qs[:1], a.k))
    res["first_search_after_remove_refresh_path_ms"] = round(t, 2)
    ix2, _, _ = build(1)
    ix2.remove(one_pct)
    t, _ = ms(lambda: ix2.search(qs[:1], a.k))
    res["first_search_after_remove_repack_path_ms"] = round(t, 2)
    same = all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) and np.array_equal(dx, dy)
               for (x, dx), (y, dy) in [(ix.search(batch, a.k), ix2.search(batch, a.k))])
    res["refresh_and_repack_results_identical"] = bool(same)
    ix2.close()
    ix.remove(ten_pct)
    ix.search(qs[:1], a.k)
    res["removed_10pct_masked_kernel"] = dict(timed_searches(ix), stat=ix.stat())
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "probe.bm25")
        t, _ = ms(lambda: ix.save(path))
        res["save"] = {"ms": round(t, 1), "bytes": os.path.getsize(path), "with_removed_documents": True}
        t, back = ms(lambda: BM25Index.load(path))
        t2, _ = ms(lambda: back.search(qs[:1], a.k))
        res["load"] = {"load_ms": round(t, 1), "first_search_with_image_upload_ms": round(t2, 1)}
        back.close()
    t, m = ms(ix.compact)
    res["compact"] = {"ms": round(t, 1), "documents_after": int((m >= 0).sum())}
    t, _ = ms(lambda: ix.search(qs[:1], a.k))
    res["first_search_after_compact_ms"] = round(t, 1)
    ix.close()
    print("BM25_PROBE_GPU " + json.dumps(res), flush=True)


def cpu_sample(a):
    """rank_bm25's get_scores + get_top_n, restated: idf table, per-document tf dicts, per query token a list comprehension over all
    documents, argsort of all scores."""
    texts = corpus(a.docs, a.vocab)[:a.cpu_sample]
    qs = queries(texts, a.cpu_queries)
    toks = [t.split() for t in texts]
    doc_freqs, df = [], {}
    for t in toks:
        f = {}
        for w in t:
            f[w] = f.get(w, 0) + 1
        doc_freqs.append(f)
        for w in f:
            df[w] = df.get(w, 0) + 1
    n = len(texts)
    dl = np.array([len(t) for t in toks], np.float64)
    avgdl = dl.sum() / n
    idf = {w: float(np.log(n - c + 0.5) - np.log(c + 0.5)) for w, c in df.items()}
    eps = 0.25 * sum(idf.values()) / len(idf)
    idf = {w: (eps if v < 0 else v) for w, v in idf.items()}
    k1, b = 1.5, 0.75
    times = []
    for q in qs:
        t0 = time.perf_counter()
        score = np.zeros(n)
        for w in q.split():
            qf = np.array([(d.get(w) or 0) for d in doc_freqs])
            score += (idf.get(w) or 0) * (qf * (k1 + 1) / (qf + k1 * (1 - b + b * dl / avgdl)))
        top = np.argsort(score)[::-1][:a.k]
        times.append((time.perf_counter() - t0) * 1e3)
        assert top.shape == (a.k,)
    med = statistics.median(times)
    return {"sample_docs": n, "queries": len(qs), "per_query_on_sample": summary(times), "scaled_linearly_to_docs": a.docs,
            "per_query_scaled_ms": round(med * a.docs / n, 2), "label": "sampled: measured on sample_docs documents, scaled by docs / sample_docs"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1_000_000)
    ap.add_argument("--vocab", type=int, default=50_000)
    ap.add_argument("--singles", type=int, default=64)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--k", type=int, default=4)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--append-reps", type=int, default=5, help="--lifecycle: legs per path and append size")
    ap.add_argument("--cpu-sample", type=int, default=100_000)
    ap.add_argument("--cpu-queries", type=int, default=8)
    ap.add_argument("--step-timeout", type=int, default=420, help="seconds the GPU step may take")
    ap.add_argument("--lifecycle", action="store_true", help="measure remove / refresh / repack / compact / save / load instead")
    ap.add_argument("--out", default=None, help="default: profiles/bm25_probe.json, or profiles/bm25_lifecycle.json with --lifecycle")
    ap.add_argument("--gpu-step", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "bm25_lifecycle.json" if a.lifecycle else "bm25_probe.json")
    if a.gpu_step:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("bm25_probe: no GPU: there is nothing to measure without one")
        print("BM25_PROBE_DEVICE " + torch.cuda.get_device_name(0), flush=True)
        return lifecycle_step(a) if a.lifecycle else gpu_step(a)
    child = subprocess.run([sys.executable, os.path.abspath(__file__), "--gpu-step"] + [x for x in sys.argv[1:] if x != "--gpu-step"],
                           capture_output=True, text=True, timeout=a.step_timeout)
    if child.returncode != 0:
        sys.stderr.write(child.stdout[-2000:] + child.stderr[-4000:])
        raise SystemExit(f"bm25_probe: the GPU step failed (exit {child.returncode}); nothing measured")
    gpu = device = None
    for ln in child.stdout.splitlines():
        if ln.startswith("BM25_PROBE_GPU "):
            gpu = json.loads(ln[len("BM25_PROBE_GPU "):])
        if ln.startswith("BM25_PROBE_DEVICE "):
            device = ln[len("BM25_PROBE_DEVICE "):]
    if a.lifecycle:
        line = json.dumps({"probe": "bm25_lifecycle", "docs": a.docs, "vocab": a.vocab, "k": a.k, "query_tokens": [8, 16], "device": device,
                           "timing": "host wall-clock around each call (searches end in a stream synchronise)", "gpu": gpu})
    else:
        line = json.dumps({"probe": "bm25", "docs": a.docs, "vocab": a.vocab, "k": a.k, "query_tokens": [8, 16], "device": device,
                           "timing": "host wall-clock around rmu_bm25_search (ends in a stream synchronise)", "gpu": gpu, "cpu": cpu_sample(a)})
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
