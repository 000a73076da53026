"""The semantic splitter's ingest step, two ways, on synthetic documents (`--docs` documents of `--sentences` sentences in the style of
tests/helpers.synth_texts) and a synthetic sentence-transformers checkpoint (tests/helpers.write_st_checkpoint, random weights: the cost
of a forward does not depend on them):

  (A) the yardstick, the reference's path restated: per document, `embed_documents(windows)` -> Python lists, then one numpy 1 x 1
      cosine_similarity per adjacent pair (langchain's: np.array of both lists, norms, X @ Y.T / outer), thresholds and assembly;
  (B) one `MI355XSemanticChunker.split_documents` call over all documents: one `embed_documents_device`, one `rmu_adjacent_cosine`.

The legs alternate A, B, A, B, ... in one process; sentence split, windows, thresholds and assembly are the same host functions on both legs,
so the difference is the embedding hand-over and the distances.  It also times the kernel alone with hipEvents (device in, device out) on
the windows' tensor and on a matrix larger than the Infinity Cache, and reports bytes / time against 8 TB/s.

  python tools/chunk_probe.py [--docs 64] [--sentences 128] [--reps 7] [--out profiles/chunk_probe.json]

Leg times are host wall-clock around calls that end synchronised.  The GPU step runs in a child process under its own time limit
(`--step-timeout`) and writes one JSON line; every entry says whether it was measured."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK_TBS = 8.0


def summary(v):
    return {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4), "n": len(v)}


def documents(n_docs, n_sentences, seed=0):
    from tests.helpers import synth_texts
    out = []
    for d in range(n_docs):
        sents = synth_texts(n_sentences, seed=seed * 100003 + d, wmin=4, wmax=24)
        out.append(" ".join(s.replace("\n", " ").rstrip(".?!,;:") + "." for s in sents))
    return out


def reference_cosine(x, y):
    """langchain_community.utils.math.cosine_similarity on two single vectors given as lists"""
    X, Y = np.array([x]), np.array([y])
    xn, yn = np.linalg.norm(X, axis=1), np.linalg.norm(Y, axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        sim = np.dot(X, Y.T) / np.outer(xn, yn)
    sim[np.isnan(sim) | np.isinf(sim)] = 0.0
    return sim[0][0]


def kernel_ms(x, reps):
    """hipEvent time of rmu_adjacent_cosine alone, device in and device out on a torch stream"""
    import torch
    from ragmeup_amd import _native as N
    lib = N.lib()
    n, dim = x.shape
    out = torch.empty(n - 1, dtype=torch.float64, device=x.device)
    s = torch.cuda.Stream()
    times = []
    torch.cuda.synchronize()
    for r in range(reps + 2):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(s)
        N.check(lib.rmu_adjacent_cosine(x.data_ptr(), n, dim, x.stride(0), N.F_Q_DEVICE | N.F_OUT_DEVICE, out.data_ptr(), s.cuda_stream),
                "rmu_adjacent_cosine")
        b.record(s)
        s.synchronize()
        if r >= 2:
            times.append(a.elapsed_time(b))
    nbytes = n * dim * 4 + (n - 1) * 8
    med = statistics.median(times)
    tbs = nbytes / (med * 1e-3) / 1e12
    return {"measured": True, "rows": n, "dim": dim, "bytes": nbytes, **summary(times), "tb_per_s": round(tbs, 4),
            "share_of_8_tb_per_s": round(tbs / HBM_PEAK_TBS, 4)}


def gpu_step(a):
    from ragmeup_amd.embeddings import MI355XEmbeddings
    from tests.helpers import write_st_checkpoint
    with tempfile.TemporaryDirectory() as tmp:
        d = os.path.join(tmp, "st")
        write_st_checkpoint(d, pooling="mean", normalize=True, max_seq_length=256, layers=6, seed=0, scale=3.0)
        emb = MI355XEmbeddings(model_dir=d)
        measure(a, emb)


def measure(a, emb):
    import torch
    from ragmeup_amd import Document
    from ragmeup_amd import chunker as C
    texts = documents(a.docs, a.sentences)
    docs = [Document(page_content=t, metadata={"doc": i}) for i, t in enumerate(texts)]
    ch = C.MI355XSemanticChunker(emb)

    def leg_a():
        out = []
        for t in texts:
            s = C.split_sentences(t)
            if not C.needs_embedding(s, "percentile"):
                out.append(list(s))
                continue
            e = emb.embed_documents(C.build_windows(s, 1))
            dist = [1 - reference_cosine(e[i], e[i + 1]) for i in range(len(e) - 1)]
            out.append(C.chunks_from_distances(s, dist, "percentile"))
        return out

    def leg_b():
        return ch.split_documents(docs)

    n_windows = sum(len(C.split_sentences(t)) for t in texts)
    ca, cb = leg_a(), leg_b()                                      # warm-up, and how far the two legs agree
    per_doc = [[] for _ in texts]
    for dd in cb:
        per_doc[dd.metadata["doc"]].append(dd.page_content)
    same = sum(x == y for x, y in zip(ca, per_doc))
    ta, tb = [], []
    for _ in range(a.reps):
        t0 = time.perf_counter(); leg_a(); ta.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter(); leg_b(); tb.append((time.perf_counter() - t0) * 1e3)
    ma, mb = statistics.median(ta), statistics.median(tb)
    windows = [w for t in texts for w in C.build_windows(C.split_sentences(t), 1)]
    E = emb.embed_documents_device(windows)
    g = torch.Generator(device="cuda").manual_seed(0)
    big = torch.randn((a.large_rows, 384), device="cuda", generator=g)
    res = {"measured": True, "windows": n_windows,
           "A_reference_path_per_document": summary(ta), "B_one_split_documents_call": summary(tb),
           "A_over_B": round(ma / mb, 3), "B_faster_than_A": bool(mb < ma), "ranges_overlap": bool(min(ta) <= max(tb) and min(tb) <= max(ta)),
           "documents_with_identical_chunks": f"{same} of {len(texts)} (a per-document forward and the batch's differ by bf16 batch-shape noise)",
           "kernel_on_the_windows": kernel_ms(E, 20), "kernel_on_a_matrix_beyond_the_infinity_cache": kernel_ms(big, 10)}
    print("CHUNK_PROBE_GPU " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--docs", type=int, default=64)
    ap.add_argument("--sentences", type=int, default=128)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--large-rows", type=int, default=1 << 19, help="rows of the 384-wide matrix of the bandwidth measurement (805 MB)")
    ap.add_argument("--step-timeout", type=int, default=540, help="seconds the GPU step may take")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "chunk_probe.json"))
    ap.add_argument("--gpu-step", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.gpu_step:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("chunk_probe: no GPU: there is nothing to measure without one")
        print("CHUNK_PROBE_DEVICE " + torch.cuda.get_device_name(0), flush=True)
        return gpu_step(a)
    child = subprocess.run([sys.executable, os.path.abspath(__file__), "--gpu-step"] + [x for x in sys.argv[1:] if x != "--gpu-step"],
                           capture_output=True, text=True, timeout=a.step_timeout)
    if child.returncode != 0:
        sys.stderr.write(child.stdout[-2000:] + child.stderr[-4000:])
        raise SystemExit(f"chunk_probe: the GPU step failed (exit {child.returncode}); nothing measured")
    gpu = device = None
    for ln in child.stdout.splitlines():
        if ln.startswith("CHUNK_PROBE_GPU "):
            gpu = json.loads(ln[len("CHUNK_PROBE_GPU "):])
        if ln.startswith("CHUNK_PROBE_DEVICE "):
            device = ln[len("CHUNK_PROBE_DEVICE "):]
    line = json.dumps({"probe": "chunk", "docs": a.docs, "generated_sentences_per_doc": a.sentences, "dim": 384, "buffer_size": 1, "type": "percentile",
                       "device": device,
                       "timing": "legs: host wall-clock per pass over all documents, same process, alternating A, B; kernel: hipEvents on one stream",
                       "gpu": gpu})
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
