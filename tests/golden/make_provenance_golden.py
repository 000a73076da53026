"""Generates tests/golden/provenance_golden.npz by RUNNING the reference's own server/provenance.py (imported from /root/reference by path,
never copied): DocumentSimilarityAttribution.compute_similarity over prepared embeddings.

sentence-transformers and langchain are not installed here, so the two names that file imports from them are minimal stand-ins: a
SentenceTransformer whose ``encode`` returns the prepared float32 rows of the texts it is given, and an empty ChatPromptTemplate.  torch and
scikit-learn are the real ones: every cosine, the average, the sum and the division are the reference's code executing unmodified, and its
scores come back as float32.  Per case the file holds the float32 embeddings, include_query and the reference's outputs.
Run in the build container only:  python tests/golden/make_provenance_golden.py
"""
import importlib.util
import os
import sys
import types

import numpy as np

REF = "/root/reference/server/provenance.py"
HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "provenance_golden.npz")
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import provenance_ref as R  # noqa: E402

DIM = 384
ROWS = {}                                                   # text -> its prepared float32 embedding


class _Model:
    def __init__(self, *a, **kw):
        pass

    def encode(self, texts):
        return np.stack([ROWS[t] for t in texts])


def _stub(name, **attrs):
    m = types.ModuleType(name)
    m.__dict__.update(attrs)
    sys.modules[name] = m


_stub("sentence_transformers", SentenceTransformer=_Model)
_stub("langchain")
_stub("langchain.prompts", ChatPromptTemplate=object)
spec = importlib.util.spec_from_file_location("ref_provenance", REF)
ref = importlib.util.module_from_spec(spec)
spec.loader.exec_module(ref)

rng = np.random.default_rng(20261019)


def unit(v):
    return v / np.linalg.norm(v)


def near(anchor, weight, n):
    """n rows: weight * anchor direction + (1 - |weight|) * a random direction, normalised"""
    return np.stack([unit(weight * unit(anchor) + (1 - abs(weight)) * unit(rng.standard_normal(DIM))) for _ in range(n)])


def case(name, n, include_query, weight=0.6, scale=1.0, zero_rows=(), all_zero=False):
    answer = unit(rng.standard_normal(DIM))
    query = unit(0.5 * answer + 0.5 * unit(rng.standard_normal(DIM)))
    docs = near(answer + query, weight, n)
    if all_zero:
        docs[:] = 0.0
    for z in zero_rows:
        docs[z] = 0.0
    return {"name": name, "include_query": include_query, "answer": (scale * answer).astype(np.float32),
            "query": (scale * query).astype(np.float32), "docs": (scale * docs).astype(np.float32)}


CASES = [
    case("query_on_5", 5, True),
    case("query_off_5", 5, False),
    case("query_on_10", 10, True),
    case("query_off_1", 1, False),
    case("query_on_2_unnormalised", 2, True, scale=3.0),
    case("query_off_7_unnormalised", 7, False, scale=0.37),
    case("zero_row_query_on", 6, True, zero_rows=(2,)),
    case("zero_row_query_off", 4, False, zero_rows=(0, 3)),
    case("negative_total_query_on", 5, True, weight=-0.6),
    case("negative_total_query_off", 3, False, weight=-0.6),
    case("zero_total_query_on", 4, True, all_zero=True),
    case("zero_total_query_off", 2, False, all_zero=True),
]

store = {"names": np.array([c["name"] for c in CASES])}
worst = (0.0, None)
for i, c in enumerate(CASES):
    ROWS.clear()
    ROWS["the answer"] = c["answer"]
    ROWS["the query"] = c["query"]
    context = [f"context {j}" for j in range(len(c["docs"]))]
    for t, row in zip(context, c["docs"]):
        ROWS[t] = row
    os.environ["attribute_include_query"] = "True" if c["include_query"] else "False"
    out = ref.DocumentSimilarityAttribution().compute_similarity("the query", context, "the answer")
    assert all(isinstance(v, np.float32) for v in out), [type(v) for v in out]
    out = np.asarray(out, dtype=np.float32)
    assert not np.isnan(out).any()
    want, _, total = R.attribute(c["docs"], c["answer"], c["query"] if c["include_query"] else None)
    assert total == 0.0 or abs(total) >= 0.25, (c["name"], total)
    n = len(context)
    eps32 = (2 * DIM + 8) * 2.0 ** -24
    bound = eps32 * (1 / abs(total) + n / total ** 2) if total > 0 else eps32
    err = float(np.abs(out.astype(np.float64) - want).max())
    print(f"{c['name']:28s} n {n:2d}  T {total:+.4f}  max |reference - restatement| {err:.3e}  bound {bound:.3e}")
    assert err <= bound
    if err > worst[0]:
        worst = (err, f"{c['name']} (dim {DIM}, n {n}, T {total:.2f})")
    store[f"c{i}_answer"], store[f"c{i}_query"], store[f"c{i}_docs"] = c["answer"], c["query"], c["docs"]
    store[f"c{i}_include_query"] = np.array(c["include_query"])
    store[f"c{i}_out"] = out
np.savez_compressed(OUT, **store)
print("observed worst", f"{worst[0]:.3e}", "at", worst[1])
print("wrote", OUT, len(CASES), "cases,", os.path.getsize(OUT), "bytes")
