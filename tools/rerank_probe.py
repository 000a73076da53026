"""The rerank step of ONE request, two ways, in one process, on a synthetic cross-encoder (tests/helpers.write_ce_checkpoint, 6 layers, random
weights: the cost of a forward does not depend on them) and synthetic texts (tests/helpers.synth_texts) whose token counts follow bench.py's
passages (clip(N(128, 32), 16, 256)):

  (a) the parent path, `ScoredCrossEncoderReranker.compress_documents`: tokenise the m (query, passage) pairs on the host, pad, copy up,
      forward, logits back, Python sort;
  (b) `MI355XRerankRetriever.compress_documents`: tokenise the query, look the passages' keys up, ONE `rmu_bert_rerank`.

at the reference's shape (one query, m = 14) and at BASELINE config C5's (64 queries x 100 passages: 64 requests of m = 100 over one pool of
passages), medians per request after warm-up (eager, capture, replay of every shape), legs alternating a, b, a, b.  It also times the
first-sight call of (b) -- passages the table has never seen, which it still tokenises -- at both shapes.

  python tools/rerank_probe.py [--reps 30] [--out profiles/rerank_one_call.md]

Times are host wall-clock around calls that end synchronised.  There is nothing to measure without a GPU."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def med(v):
    return statistics.median(v)


def passages(n, tok, seed):
    """n texts of about clip(N(128, 32), 16, 256) tokens each"""
    from tests.helpers import synth_texts
    probe = synth_texts(200, seed=seed, wmin=40, wmax=40)
    per_word = float(np.mean(tok.encode(probe, None, max_len=512)[2] - 2)) / 40.0
    rng = np.random.default_rng(seed)
    want = np.clip(np.rint(rng.normal(128, 32, n)), 16, 256)
    out = []
    for i, t in enumerate(want):
        w = max(1, int(round(t / per_word)))
        out.append(synth_texts(1, seed=seed * 1000003 + i, wmin=w, wmax=w)[0])
    return out


def shape_rows(name, ce, requests, reps, fresh_sets):
    """requests: [(query, [texts])]; fresh_sets: the same requests over texts the table has not seen (one set per first-sight sample)"""
    from ragmeup_amd import Document, MI355XRerankRetriever, ScoredCrossEncoderReranker
    comp = ScoredCrossEncoderReranker(model=ce, top_n=3)
    r = MI355XRerankRetriever(base_compressor=comp, base_retriever=None)
    docs = [(q, [Document(page_content=t, metadata={}) for t in texts]) for q, texts in requests]
    for _ in range(3):
        for q, d in docs:
            a, b = comp.compress_documents(d, q), r.compress_documents(d, q)
            assert [(x.page_content, x.metadata) for x in a] == [(x.page_content, x.metadata) for x in b]
    ta, tb = [], []
    for _ in range(reps):
        for q, d in docs:
            t0 = time.perf_counter(); comp.compress_documents(d, q); ta.append((time.perf_counter() - t0) * 1e3)
            t0 = time.perf_counter(); r.compress_documents(d, q); tb.append((time.perf_counter() - t0) * 1e3)
    tf = []
    for q, texts in fresh_sets:                                    # (the shapes are warm: what is new is the passages)
        d = [Document(page_content=t, metadata={}) for t in texts]
        t0 = time.perf_counter(); r.compress_documents(d, q); tf.append((time.perf_counter() - t0) * 1e3)
    tokens = ce.tokenizer.encode([t for _, texts in requests for t in texts], None, max_len=512)[2] - 2
    return {"shape": name, "requests": len(requests), "m": len(requests[0][1]), "mean_passage_tokens": round(float(tokens.mean()), 1),
            "a_compressor_ms": round(med(ta), 4), "a_min_ms": round(min(ta), 4), "b_one_call_ms": round(med(tb), 4), "b_min_ms": round(min(tb), 4),
            "b_first_sight_ms": round(med(tf), 4), "a_over_b": round(med(ta) / med(tb), 3), "samples": len(ta), "first_sight_samples": len(tf)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rerank_one_call.md"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("rerank_probe: no GPU: there is nothing to measure without one")
    from ragmeup_amd.embeddings import MI355XCrossEncoder
    from tests.helpers import synth_texts, write_ce_checkpoint
    with tempfile.TemporaryDirectory() as tmp:
        d = os.path.join(tmp, "ce")
        write_ce_checkpoint(d, layers=6)
        ce = MI355XCrossEncoder(model_dir=d)
        tok = ce.tokenizer
        queries = [" ".join(t.split()[:10]) for t in synth_texts(64, seed=5, wmin=12, wmax=12)]
        rows = []
        pool = passages(14, tok, seed=1)
        fresh = [(queries[0], passages(14, tok, seed=100 + i)) for i in range(8)]
        rows.append(shape_rows("reference: 1 query x 14 passages", ce, [(queries[0], pool)], a.reps * 4, fresh))
        pool = passages(2000, tok, seed=2)
        rng = np.random.default_rng(9)
        reqs = [(q, [pool[j] for j in rng.choice(len(pool), 100, replace=False)]) for q in queries]
        fresh = [(queries[i], passages(100, tok, seed=200 + i)) for i in range(8)]
        rows.append(shape_rows("C5: 64 queries x 100 passages, per query", ce, reqs, max(1, a.reps // 10), fresh))
    dev = torch.cuda.get_device_name(0)
    lines = ["# Rerank in one call: what it saves per request", "",
             f"`tools/rerank_probe.py` on {dev}: synthetic 6-layer cross-encoder, synthetic passages (token counts as bench.py's), host wall-clock",
             "per request around calls that end synchronised, medians after warm-up, legs alternating in one process.", "",
             "(a) `ScoredCrossEncoderReranker.compress_documents` (tokenise m pairs, pad, copy, forward, sort on the host); (b)",
             "`MI355XRerankRetriever.compress_documents` (tokenise the query, keys from the table, one `rmu_bert_rerank`); first sight: (b) over",
             "passages the table has not seen, which it still tokenises.", "",
             "| shape | passage tokens (mean) | (a) ms | (b) ms | (a) / (b) | (b) first sight ms | samples |", "|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append(f"| {r['shape']} | {r['mean_passage_tokens']} | {r['a_compressor_ms']} (min {r['a_min_ms']}) | {r['b_one_call_ms']} (min {r['b_min_ms']}) | "
                     f"{r['a_over_b']} | {r['b_first_sight_ms']} | {r['samples']} / {r['first_sight_samples']} |")
    lines += ["", "```json", json.dumps({"probe": "rerank_one_call", "device": dev, "rows": rows}), "```", ""]
    text = "\n".join(lines)
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
