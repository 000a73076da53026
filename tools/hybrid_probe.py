"""The ensemble's retrieval step, two ways, on one synthetic corpus: `--docs` documents from tools/bm25_probe.py's generator in a BM25 index
beside `--docs` x 384 random unit rows in a flat index (row i and document i hold the same text), k_sparse = k_dense = 4, fetch_k = 20,
lambda = 0.5, weights (0.5, 0.5).  Per single query and per batch of 64 and of 1024 queries it times

  (a) the two member calls + the host fusion: rmu_bm25_search, rmu_index_search_mmr, the ids turned into Documents and
      ragmeup_amd.ensemble.weighted_reciprocal_rank over them (what MI355XEnsembleRetriever does per request), and
  (b) the one call: rmu_hybrid_search and the fused ids turned into Documents (what MI355XHybridRetriever does),

in the same process, alternating (a), (b), (a): the second (a) pass gives the run-to-run spread the comparison is read against.  The query
vectors are made up front (embedding is the same work on both paths).  Both paths must return the same documents; the probe checks that.

  python tools/hybrid_probe.py [--docs 1000000] [--vocab 50000] [--reps 30] [--out profiles/hybrid_probe.json]

Times are host wall-clock around calls that end in a stream synchronise.  The GPU step runs in a child process under its own time limit
(`--step-timeout`) and writes one JSON line."""
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

SIZES = (1, 64, 1024)
K_SPARSE, FETCH_K, K_DENSE, LAMBDA, WEIGHTS, C = 4, 20, 4, 0.5, (0.5, 0.5), 60


def summary(v):
    return {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4), "n": len(v)}


def gpu_step(a):
    import torch
    from bm25_probe import corpus, queries
    from ragmeup_amd import FlatIndex
    from ragmeup_amd._lc import Document
    from ragmeup_amd.bm25 import BM25Index
    from ragmeup_amd.ensemble import weighted_reciprocal_rank
    from ragmeup_amd.hybrid import HybridIndex, content_keys
    texts = corpus(a.docs, a.vocab)
    docs = [Document(page_content=t, metadata={"doc": i}) for i, t in enumerate(texts)]
    bm25 = BM25Index()
    for lo in range(0, len(texts), 100_000):
        bm25.add_texts(texts[lo:lo + 100_000])
    idx = FlatIndex(384, capacity_hint=a.docs)
    g = torch.Generator(device="cuda").manual_seed(0)
    for lo in range(0, a.docs, 100_000):
        x = torch.randn((min(100_000, a.docs - lo), 384), device="cuda", generator=g)
        idx.add(x / x.norm(dim=1, keepdim=True))
    keys = content_keys(texts, {})
    h = HybridIndex(bm25, idx)
    h.set_keys(0, 0, keys)
    h.set_keys(1, 0, keys)
    rng = np.random.default_rng(5)
    res = {}

    def two_calls(qs, qv):
        _, d = bm25.search(qs, K_SPARSE)
        r, _ = idx.search_mmr(qv, FETCH_K, K_DENSE, LAMBDA)
        return [weighted_reciprocal_rank([[docs[i] for i in dd if i >= 0], [docs[i] for i in rr if i >= 0]], WEIGHTS, C)
                for dd, rr in zip(d.tolist(), r.tolist())]

    def one_call(qs, qv):
        _, ids, _ = h.search(qv, qs, K_SPARSE, FETCH_K, K_DENSE, LAMBDA, WEIGHTS, C)
        return [[docs[i] for i in row if i >= 0] for row in ids.tolist()]

    def timed(fn, batches):
        out = []
        for qs, qv in batches:
            t0 = time.perf_counter()
            fn(qs, qv)
            out.append((time.perf_counter() - t0) * 1e3)
        return out

    for nq in SIZES:
        reps = a.reps if nq < 1024 else max(5, a.reps // 3)
        batches = []
        for r in range(reps):
            qv = rng.standard_normal((nq, 384)).astype(np.float32)
            batches.append((queries(texts, nq, seed=100 * nq + r), qv / np.linalg.norm(qv, axis=1, keepdims=True)))
        same = all([[d.metadata["doc"] for d in x] for x in two_calls(*b)] == [[d.metadata["doc"] for d in x] for x in one_call(*b)] for b in batches[:3])
        a1, b1, a2 = timed(two_calls, batches), timed(one_call, batches), timed(two_calls, batches)
        m1, mb, m2 = statistics.median(a1), statistics.median(b1), statistics.median(a2)
        spread = abs(m1 - m2)
        res[f"nq_{nq}"] = {"measured": True, "two_calls_plus_host_fusion": summary(a1), "one_call": summary(b1),
                           "two_calls_plus_host_fusion_again": summary(a2), "run_to_run_spread_ms": round(spread, 4),
                           "one_call_minus_two_calls_ms": round(mb - min(m1, m2), 4),
                           "one_call_slower_beyond_spread": bool(mb > max(m1, m2) + spread), "same_documents": bool(same)}
    h.close()
    idx.close()
    bm25.close()
    print("HYBRID_PROBE_GPU " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=1_000_000)
    ap.add_argument("--vocab", type=int, default=50_000)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--step-timeout", type=int, default=540, help="seconds the GPU step may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hybrid_probe.json"))
    ap.add_argument("--gpu-step", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.gpu_step:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("hybrid_probe: no GPU: there is nothing to measure without one")
        print("HYBRID_PROBE_DEVICE " + torch.cuda.get_device_name(0), flush=True)
        return gpu_step(a)
    child = subprocess.run([sys.executable, os.path.abspath(__file__), "--gpu-step"] + [x for x in sys.argv[1:] if x != "--gpu-step"],
                           capture_output=True, text=True, timeout=a.step_timeout)
    if child.returncode != 0:
        sys.stderr.write(child.stdout[-2000:] + child.stderr[-4000:])
        raise SystemExit(f"hybrid_probe: the GPU step failed (exit {child.returncode}); nothing measured")
    gpu = device = None
    for ln in child.stdout.splitlines():
        if ln.startswith("HYBRID_PROBE_GPU "):
            gpu = json.loads(ln[len("HYBRID_PROBE_GPU "):])
        if ln.startswith("HYBRID_PROBE_DEVICE "):
            device = ln[len("HYBRID_PROBE_DEVICE "):]
    line = json.dumps({"probe": "hybrid", "docs": a.docs, "vocab": a.vocab, "dim": 384, "k_sparse": K_SPARSE, "fetch_k": FETCH_K, "k_dense": K_DENSE,
                       "lambda_mult": LAMBDA, "weights": list(WEIGHTS), "c": C, "query_tokens": [8, 16], "device": device,
                       "timing": "host wall-clock per call, same process, passes in the order (a) two calls + host fusion, (b) one call, (a) again",
                       "gpu": gpu})
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
