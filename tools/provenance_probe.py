"""Similarity provenance of ONE request (`--contexts` contexts, the query included), two ways, on synthetic texts (tests/helpers.synth_texts)
and a synthetic sentence-transformers checkpoint (tests/helpers.write_st_checkpoint, random weights: the cost of a forward does not depend on
them):

  (A) the yardstick, the reference's shape (server/provenance.py:171-202): three embed calls (answer, contexts, query), the rows to the host,
      2 n numpy cosines on 1 x dim matrices (sklearn's: normalise both, dot), a Python sum and a division;
  (B) one `DocumentSimilarityAttribution.compute_similarity`: one forward over all texts and the attribution kernel behind it
      (`rmu_bert_attribute`), one synchronisation.

The legs alternate A, B, A, B, ... in one process.  It also takes the hipEvent time of `rmu_attribution` alone on the request's embeddings
(device in, device out, on one stream: the upload of the 5-int group table and the kernel).

  python tools/provenance_probe.py [--contexts 10] [--reps 50] [--out profiles/provenance_probe.json]

Leg times are host wall-clock around calls that end synchronised.  There is nothing to measure without a GPU."""
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


def summary(v):
    return {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4), "n": len(v)}


def host_cosine(a, b):
    """sklearn.metrics.pairwise.cosine_similarity([a], [b])[0][0]: both rows normalised (a zero row stays zero), then the dot"""
    X, Y = np.asarray([a], dtype=np.float32), np.asarray([b], dtype=np.float32)
    xn, yn = np.linalg.norm(X, axis=1, keepdims=True), np.linalg.norm(Y, axis=1, keepdims=True)
    xn[xn == 0] = 1
    yn[yn == 0] = 1
    return ((X / xn) @ (Y / yn).T)[0][0]


def kernel_ms(x, groups, reps):
    import torch
    from ragmeup_amd import _native as N
    lib = N.lib()
    n, dim = x.shape
    total = int(groups[:, 3].sum())
    out = torch.empty(total, dtype=torch.float64, device=x.device)
    sims = torch.empty((total, 2), dtype=torch.float64, device=x.device)
    s = torch.cuda.Stream()
    times = []
    torch.cuda.synchronize()
    for r in range(reps + 3):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(s)
        N.check(lib.rmu_attribution(x.data_ptr(), n, dim, x.stride(0), groups.ctypes.data, len(groups), N.F_Q_DEVICE | N.F_OUT_DEVICE,
                                    out.data_ptr(), sims.data_ptr(), s.cuda_stream), "rmu_attribution")
        b.record(s)
        s.synchronize()
        if r >= 3:
            times.append(a.elapsed_time(b))
    return {"rows": n, "dim": dim, "documents": total, **summary(times)}


def measure(a, emb):
    from ragmeup_amd.provenance import DocumentSimilarityAttribution, build_request_table
    from tests.helpers import synth_texts
    texts = synth_texts(a.contexts + 2, seed=3, wmin=8, wmax=40)
    query, answer, context = texts[0], texts[1], texts[2:]
    attributor = DocumentSimilarityAttribution(emb, include_query=True)

    def leg_a():
        answer_e = np.asarray(emb.embed_documents([answer])[0], dtype=np.float32)
        context_e = np.asarray(emb.embed_documents(context), dtype=np.float32)
        query_e = np.asarray(emb.embed_documents([query])[0], dtype=np.float32)
        s = [(host_cosine(d, answer_e) + host_cosine(d, query_e)) / 2 for d in context_e]
        t = sum(s)
        return [v / t for v in s] if t > 0 else s

    def leg_b():
        return attributor.compute_similarity(query, context, answer)

    for _ in range(3):                                             # warm-up: eager, capture, replay of every shape
        ra, rb = leg_a(), leg_b()
    ta, tb = [], []
    for _ in range(a.reps):
        t0 = time.perf_counter(); leg_a(); ta.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter(); leg_b(); tb.append((time.perf_counter() - t0) * 1e3)
    ma, mb = statistics.median(ta), statistics.median(tb)
    all_texts, groups, _ = build_request_table([(query, context, answer)], True)
    E = emb.embed_documents_device(all_texts)
    return {"contexts": a.contexts, "include_query": True, "path_of_B": attributor.last_path,
            "A_three_embed_calls_and_host_cosines": summary(ta), "B_one_compute_similarity": summary(tb),
            "A_over_B": round(ma / mb, 3), "B_faster_than_A": bool(mb < ma), "ranges_overlap": bool(min(ta) <= max(tb) and min(tb) <= max(ta)),
            "max_abs_score_difference_A_B": float(np.abs(np.asarray(ra, dtype=np.float64) - np.asarray(rb)).max()),
            "kernel_alone_table_upload_and_launch": kernel_ms(E, groups, a.reps)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--contexts", type=int, default=10)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "provenance_probe.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("provenance_probe: no GPU: there is nothing to measure without one")
    from ragmeup_amd.embeddings import MI355XEmbeddings
    from tests.helpers import write_st_checkpoint
    with tempfile.TemporaryDirectory() as tmp:
        d = os.path.join(tmp, "st")
        write_st_checkpoint(d, pooling="mean", normalize=True, max_seq_length=256, layers=6, seed=0, scale=3.0)
        gpu = measure(a, MI355XEmbeddings(model_dir=d))
    line = json.dumps({"probe": "provenance", "dim": 384, "device": torch.cuda.get_device_name(0),
                       "timing": "legs: host wall-clock per request, same process, alternating A, B; kernel: hipEvents on one stream", "gpu": gpu})
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
