"""One small call into every unit of librmu that owns a thread-local context (index, top-k merge, BM25, RRF, adjacent cosine, attribution,
rerank select), from host arrays so that every device and pinned buffer of every context is allocated: on the main thread, on two worker
threads started and joined one after the other (each join runs the thread's context destructors), on the main thread again, then a normal
process exit (the main thread's destructors, then the static ones).  Prints `ok` last.  For tests/test_thread_exit_gpu.py."""
import ctypes
import os
import sys
import threading

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ragmeup_amd import BM25Index, FlatIndex, topk_merge  # noqa: E402
from ragmeup_amd import _native as N  # noqa: E402
from ragmeup_amd.chunker import adjacent_cosine  # noqa: E402
from ragmeup_amd.provenance import attribution  # noqa: E402

lib = N.lib()
rng = np.random.default_rng(7)
x = rng.standard_normal((256, 384)).astype(np.float32)
x /= np.linalg.norm(x, axis=1, keepdims=True)
q = x[[5, 77, 200]] + 0.05 * rng.standard_normal((3, 384)).astype(np.float32)
subset = np.arange(3, 256, 16, dtype=np.int64)                       # 16 ascending ids
part_s = -np.sort(-rng.standard_normal((2, 3, 4)).astype(np.float32), axis=2)
part_r = rng.permutation(24).astype(np.int64).reshape(2, 3, 4)
texts = ["the quick brown fox", "jumps over the lazy dog", "a fox is a wild animal", "dogs are loyal", "the dog barks at the fox",
         "lazy afternoons", "quick thinking wins", "brown bread and butter"]
rrf_keys = np.array([[[3, 1, 4, 2]], [[2, 7, 3, 9]]], dtype=np.int64)   # [lists = 2, nq = 1, depth = 4]
rows5 = x[:5].copy()
rows6 = x[10:16].copy()
groups = np.array([[0, 1, 2, 4]], dtype=np.int32)                    # answer row 0, query row 1, documents 2 .. 5
logits = np.array([[0.5, -1.0, 2.0, 0.5], [3.0, 3.0, -0.0, 0.0]], dtype=np.float32)
sel_keys = np.array([[10, 11, -1, 13], [20, 21, 22, 23]], dtype=np.int64)

index = FlatIndex(384)
index.add(x)
bm25 = BM25Index()
bm25.add_texts(texts)


def calls():
    out = []
    out += index.search(q, 4)
    out += index.search(q, 4, rows=subset)
    out += topk_merge(part_s, part_r)
    out += bm25.search(["quick fox", "lazy dog barks"], 3)
    s, k, r = np.empty((1, 8), np.float64), np.empty((1, 8), np.int64), np.empty((1, 8), np.int32)
    N.check(lib.rmu_rrf_fuse(rrf_keys.ctypes.data, 2, 1, 4, (ctypes.c_double * 2)(0.5, 0.5), 60, 8, 0, s.ctypes.data, k.ctypes.data, r.ctypes.data, 0),
            "rmu_rrf_fuse")
    out += [s, k, r]
    out.append(adjacent_cosine(rows5))
    out += attribution(rows6, groups)
    pos, sc = np.empty((2, 3), np.int32), np.empty((2, 3), np.float32)
    N.check(lib.rmu_rerank_select(logits.ctypes.data, sel_keys.ctypes.data, 2, 4, 3, 0, pos.ctypes.data, sc.ctypes.data, 0), "rmu_rerank_select")
    out += [pos, sc]
    return [np.asarray(a).tobytes() for a in out]


main = calls()
assert len(main) == 16 and all(main)
for _ in range(2):
    got = []
    t = threading.Thread(target=lambda: got.append(calls()))
    t.start()
    t.join()                                                          # the worker's contexts are destroyed here
    assert got and got[0] == main, "a worker thread's results differ from the main thread's"
assert calls() == main, "the main thread's results changed after the workers exited"
index.close()
bm25.close()
print("ok", flush=True)
