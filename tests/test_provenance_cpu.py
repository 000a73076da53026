"""CPU: similarity provenance without a GPU -- the fp64 restatement (tests/provenance_ref.py) against the reference's own outputs
(tests/golden/provenance_golden.npz, made by tests/golden/make_provenance_golden.py), the argument validation of rmu_attribution and
rmu_bert_attribute (before any HIP call), the host half of ragmeup_amd/provenance.py and the factory hook.

Bound of the restatement against the reference, derived from the reference's arithmetic (never measured): the reference's cosine is a float32
dot of `dim` terms over two float32-normalised rows, eps32 = (2 dim + 8) 2**-24 per cosine and hence per unnormalised score (the average of
two); a normalised score s / T moves by at most eps32 / |T| for its own error plus |s| n eps32 / T**2 <= n eps32 / T**2 for the error of the
sum: eps32 (1 / |T| + n / T**2).  The generator prints the observed worst: 1.3e-7 on an unnormalised score (dim 384, n = 3, T = -2.27; eps32 =
4.6e-5) and 3.9e-8 on a normalised one (n = 4, T = 1.54; bound 1.1e-4)."""
import ctypes
import os

import numpy as np
import pytest

from tests import provenance_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "provenance_golden.npz")


def golden_cases():
    z = np.load(GOLDEN)
    for i, name in enumerate(z["names"]):
        yield {"name": str(name), "answer": z[f"c{i}_answer"], "query": z[f"c{i}_query"], "docs": z[f"c{i}_docs"],
               "include_query": bool(z[f"c{i}_include_query"]), "out": z[f"c{i}_out"]}


# ---- the restatement against the reference ------------------------------------------------------------------------------------------------------
def test_restatement_equals_the_reference_outputs_within_the_derived_bound():
    seen = set()
    n_cases = 0
    for c in golden_cases():
        n_cases += 1
        docs, out = c["docs"], c["out"]
        n, dim = docs.shape
        assert dim == 384 and 1 <= n <= 10 and out.dtype == np.float32 and out.shape == (n,)
        assert not any(np.isnan(a).any() for a in (docs, c["answer"], c["query"], out))
        want, _, total = R.attribute(docs, c["answer"], c["query"] if c["include_query"] else None)
        assert total == 0.0 or abs(total) >= 0.25, (c["name"], total)
        eps32 = (2 * dim + 8) * 2.0 ** -24
        bound = eps32 * (1 / abs(total) + n / total ** 2) if total > 0 else eps32
        err = float(np.abs(out.astype(np.float64) - want).max())
        print(f"{c['name']}: n {n} T {total:+.4f} max |reference - restatement| {err:.3e} bound {bound:.3e}")
        assert err <= bound, c["name"]
        seen.add((c["include_query"], "neg" if total < 0 else "zero" if total == 0 else "pos"))
        if (docs == 0).all(axis=1).any() and total != 0:
            seen.add("zero row")
        if total > 0:
            assert abs(float(want.sum()) - 1.0) <= 1e-12
        if total == 0:
            assert (out == 0).all() and (want == 0).all()
    assert n_cases >= 10
    assert seen >= {(q, t) for q in (True, False) for t in ("neg", "zero", "pos")} | {"zero row"}
    assert os.path.getsize(GOLDEN) <= max(os.path.getsize(os.path.join(os.path.dirname(GOLDEN), f)) for f in os.listdir(os.path.dirname(GOLDEN))
                                          if f != "provenance_golden.npz")


# ---- ABI ------------------------------------------------------------------------------------------------------------------------------------
def _table(*rows):
    return np.asarray(rows, dtype=np.int32).reshape(-1, 4)


def test_attribution_rejects_every_invalid_argument_without_a_gpu(librmu):
    x = np.zeros((6, 8), np.float32)
    scores = np.zeros(8, np.float64)
    sims = np.zeros((8, 2), np.float64)
    ok = _table((0, 1, 2, 4))
    xp, sp, mp, gp = x.ctypes.data, scores.ctypes.data, sims.ctypes.data, ok.ctypes.data
    f = librmu.rmu_attribution

    def g(*rows):
        t = _table(*rows)
        keep.append(t)
        return t.ctypes.data, len(t)

    keep = []
    bad = {
        "null x": (None, 6, 8, 8, gp, 1, 0, sp, mp, 0),
        "null groups": (xp, 6, 8, 8, None, 1, 0, sp, mp, 0),
        "null groups, no group": (xp, 6, 8, 8, None, 0, 0, sp, mp, 0),
        "null scores": (xp, 6, 8, 8, gp, 1, 0, None, mp, 0),
        "unknown flag": (xp, 6, 8, 8, gp, 1, 4, sp, mp, 0),
        "unknown high flag": (xp, 6, 8, 8, gp, 1, 1 << 31, sp, mp, 0),
        "rows-device flag": (xp, 6, 8, 8, gp, 1, 8, sp, mp, 0),
        "dim 0": (xp, 6, 0, 8, gp, 1, 0, sp, mp, 0),
        "dim < 0": (xp, 6, -1, 8, gp, 1, 0, sp, mp, 0),
        "dim > 3072": (xp, 6, 3073, 4096, gp, 1, 0, sp, mp, 0),
        "stride < dim": (xp, 6, 8, 7, gp, 1, 0, sp, mp, 0),
        "stride < 0": (xp, 6, 8, -8, gp, 1, 0, sp, mp, 0),
        "n 0": (xp, 0, 8, 8, gp, 1, 0, sp, mp, 0),
        "n < 0": (xp, -3, 8, 8, gp, 1, 0, sp, mp, 0),
        "n * stride overflows": (xp, 1 << 40, 8, 1 << 40, gp, 1, 0, sp, mp, 0),
        "n_groups < 0": (xp, 6, 8, 8, gp, -1, 0, sp, mp, 0),
        "answer row < 0": (xp, 6, 8, 8, *g((-1, 1, 2, 4)), 0, sp, mp, 0),
        "answer row == n": (xp, 6, 8, 8, *g((6, 1, 2, 4)), 0, sp, mp, 0),
        "query row == n": (xp, 6, 8, 8, *g((0, 6, 2, 4)), 0, sp, mp, 0),
        "query row -2": (xp, 6, 8, 8, *g((0, -2, 2, 4)), 0, sp, mp, 0),
        "first row < 0": (xp, 6, 8, 8, *g((0, 1, -1, 2)), 0, sp, mp, 0),
        "first row == n": (xp, 6, 8, 8, *g((0, 1, 6, 0)), 0, sp, mp, 0),
        "n_docs < 0": (xp, 6, 8, 8, *g((0, 1, 2, -1)), 0, sp, mp, 0),
        "rows past n": (xp, 6, 8, 8, *g((0, 1, 2, 5)), 0, sp, mp, 0),
        "rows past n, int32 edge": (xp, 6, 8, 8, *g((0, 1, 2, 2 ** 31 - 1)), 0, sp, mp, 0),
        "second group bad": (xp, 6, 8, 8, *g((0, 1, 2, 4), (0, 1, 5, 2)), 0, sp, mp, 0),
        "sum of n_docs > int32": (xp, 1 << 31, 8, 8, *g((0, -1, 0, 2 ** 31 - 1), (0, -1, 0, 1)), 0, sp, mp, 0),
    }
    for what, args in bad.items():
        assert f(*args) == -1, what
        msg = librmu.rmu_last_error()
        assert msg.startswith(b"rmu_attribution:") and len(msg) > 20, (what, msg)
    assert (scores == 0).all() and (sims == 0).all()


def test_attribution_without_documents_is_no_work(librmu):
    """n_groups == 0, and groups with n_docs == 0 only: valid, nothing written, nothing launched -- OK on a machine without a GPU."""
    x = np.ones((3, 8), np.float32)
    scores = np.full(2, 7.0)
    sims = np.full((2, 2), 7.0)
    t = _table((0, 1, 2, 0), (1, -1, 0, 0))
    for n_groups in (0, 2):
        assert librmu.rmu_attribution(x.ctypes.data, 3, 8, 8, t.ctypes.data, n_groups, 0, scores.ctypes.data, sims.ctypes.data, 0) == 0
        assert librmu.rmu_attribution(x.ctypes.data, 3, 8, 8, t.ctypes.data, n_groups, 0, scores.ctypes.data, None, 0) == 0
    assert (scores == 7.0).all() and (sims == 7.0).all()


def test_bert_attribute_rejects_every_invalid_argument_without_a_gpu(librmu):
    """No model exists without a GPU: the arguments are checked in front of the handle, so every case below fails on its own account and
    the valid call fails on the null handle alone."""
    ids = np.zeros((4, 16), np.int32)
    lens = np.full(4, 3, np.int32)
    scores = np.zeros(4, np.float64)
    ok = _table((0, 1, 2, 2))
    ip, lp, sp, gp = ids.ctypes.data, lens.ctypes.data, scores.ctypes.data, ok.ctypes.data
    f = librmu.rmu_bert_attribute
    keep = []

    def g(*rows):
        t = _table(*rows)
        keep.append(t)
        return t.ctypes.data, len(t)

    fake = ctypes.c_void_p(8)       # never dereferenced: each of these fails before the handle is looked at
    bad = {
        "null ids": (fake, None, None, lp, 4, 16, 0, gp, 1, sp, None, None),
        "null lens": (fake, ip, None, None, 4, 16, 0, gp, 1, sp, None, None),
        "null groups": (fake, ip, None, lp, 4, 16, 0, None, 1, sp, None, None),
        "null scores": (fake, ip, None, lp, 4, 16, 0, gp, 1, None, None, None),
        "batch 0": (fake, ip, None, lp, 0, 16, 0, gp, 1, sp, None, None),
        "batch < 0": (fake, ip, None, lp, -4, 16, 0, gp, 1, sp, None, None),
        "cross-encoder mode": (fake, ip, None, lp, 4, 16, 1, gp, 1, sp, None, None),
        "token mode": (fake, ip, None, lp, 4, 16, 3, gp, 1, sp, None, None),
        "n_groups < 0": (fake, ip, None, lp, 4, 16, 0, gp, -1, sp, None, None),
        "answer row == batch": (fake, ip, None, lp, 4, 16, 0, *g((4, 1, 2, 2)), sp, None, None),
        "query row == batch": (fake, ip, None, lp, 4, 16, 0, *g((0, 4, 2, 2)), sp, None, None),
        "rows past the batch": (fake, ip, None, lp, 4, 16, 0, *g((0, 1, 2, 3)), sp, None, None),
        "n_docs < 0": (fake, ip, None, lp, 4, 16, 2, *g((0, 1, 2, -2)), sp, None, None),
        "null model": (None, ip, None, lp, 4, 16, 0, gp, 1, sp, None, None),
    }
    for what, args in bad.items():
        assert f(*args) == -1, what
        msg = librmu.rmu_last_error()
        assert msg.startswith(b"rmu_bert_attribute:") and len(msg) > 24, (what, msg)
    assert (scores == 0).all()


def test_exported_from_the_package():
    import ragmeup_amd
    from ragmeup_amd import provenance as P
    assert ragmeup_amd.DocumentSimilarityAttribution is P.DocumentSimilarityAttribution is P.MI355XSimilarityAttribution
    assert ragmeup_amd.MI355XSimilarityAttribution is P.MI355XSimilarityAttribution
    assert {"DocumentSimilarityAttribution", "MI355XSimilarityAttribution"} <= set(ragmeup_amd.__all__)
    for m in ("compute_similarity", "compute_similarity_batch"):
        assert callable(getattr(P.DocumentSimilarityAttribution, m))


# ---- the host half ------------------------------------------------------------------------------------------------------------------------------
class _Doc:
    def __init__(self, text):
        self.page_content = text


def test_group_table_construction_equals_the_restatement():
    from ragmeup_amd import provenance as P
    requests = [("q0", ["a", "b", "c"], "ans0"), ("q1", [], "ans1"), ("q2", ["d"], "ans2"), ("q0", ["a", "e"], "ans3")]
    for include_query in (True, False):
        texts, groups, owner = P.build_request_table(requests, include_query)
        rtexts, rgroups = R.request_rows(requests, include_query)
        assert texts == rtexts and groups.tolist() == rgroups and owner == [0, 2, 3]
        assert groups.dtype == np.int32 and groups.shape == (3, 4)
    texts, groups, _ = P.build_request_table(requests, True)
    assert texts == ["ans0", "q0", "a", "b", "c", "ans2", "q2", "d", "ans3", "q0", "a", "e"]
    assert groups.tolist() == [[0, 1, 2, 3], [5, 6, 7, 1], [8, 9, 10, 2]]
    texts, groups, _ = P.build_request_table(requests, False)
    assert texts == ["ans0", "a", "b", "c", "ans2", "d", "ans3", "a", "e"]
    assert groups.tolist() == [[0, -1, 1, 3], [4, -1, 5, 1], [6, -1, 7, 2]]
    # documents are taken by their page_content; nothing at all gives an empty [0, 4] table
    assert P.build_request_table([("q", [_Doc("x"), "y"], "a")], False)[0] == ["a", "x", "y"]
    texts, groups, owner = P.build_request_table([("q", [], "a")], True)
    assert texts == [] and groups.shape == (0, 4) and owner == []


class _Never:
    def embed_documents(self, texts):
        raise AssertionError("embedded")


def test_an_empty_context_returns_an_empty_list_and_embeds_nothing():
    from ragmeup_amd.provenance import DocumentSimilarityAttribution
    a = DocumentSimilarityAttribution(_Never())
    assert a.compute_similarity("q", [], "answer") == []
    assert a.compute_similarity_batch([("q", [], "a"), ("r", (), "b")]) == [[], []]
    assert a.compute_similarity_batch([]) == []


@pytest.mark.parametrize("value,want", [(None, True), ("False", False), ("True", True), ("false", True), ("", True), ("0", True)])
def test_include_query_is_read_from_the_reference_s_variable_at_call_time(monkeypatch, value, want):
    from ragmeup_amd import provenance as P
    monkeypatch.delenv("attribute_include_query", raising=False)
    monkeypatch.setenv("provenance_include_query", "False")          # the template's name: not the one the reference reads
    a = P.DocumentSimilarityAttribution(_Never())                    # built BEFORE the variable is set: read per call
    if value is not None:
        monkeypatch.setenv("attribute_include_query", value)
    assert a._include_query() is want and P.include_query_from_env() is want
    assert P.include_query_from_env({} if value is None else {"attribute_include_query": value}) is want
    assert P.DocumentSimilarityAttribution(_Never(), include_query=True)._include_query() is True
    assert P.DocumentSimilarityAttribution(_Never(), include_query=False)._include_query() is False


class _Compressor:
    def __init__(self):
        self.calls = []

    def compress_documents(self, documents, query):
        self.calls.append((list(documents), query))
        return ["scored"]


@pytest.mark.parametrize("value,text", [("True", "the query\nthe answer"), ("False", "the answer"), (None, "the answer")])
def test_rerank_provenance_scores_against_the_answer_or_query_and_answer(monkeypatch, value, text):
    from ragmeup_amd.provenance import compute_rerank_provenance
    monkeypatch.delenv("attribute_include_query", raising=False)
    if value is not None:
        monkeypatch.setenv("attribute_include_query", value)
    c = _Compressor()
    docs = [_Doc("a"), _Doc("b")]
    assert compute_rerank_provenance(c, "the query", docs, "the answer") == ["scored"]
    assert c.calls == [(docs, text)]


# ---- factory ------------------------------------------------------------------------------------------------------------------------------------
def test_provenance_from_env_for_every_method(tmp_path, monkeypatch):
    from ragmeup_amd import factory
    from ragmeup_amd.provenance import DocumentSimilarityAttribution

    class Spec:
        path = str(tmp_path / "st")

    class Emb:
        spec = Spec()

    os.makedirs(Spec.path)
    emb = Emb()
    for method in ("rerank", None, "none", "Similarity", ""):
        env = {} if method is None else {"provenance_method": method}
        assert factory.provenance_from_env(env, embeddings=emb) is None
    for method in ("attention", "llm"):
        with pytest.raises(ValueError, match="LLM"):
            factory.provenance_from_env({"provenance_method": method}, embeddings=emb)
    # similarity over the directory the embeddings object serves: that object is reused (by another spelling of the path as well)
    for path in (Spec.path, os.path.join(Spec.path, "..", "st")):
        a = factory.provenance_from_env({"provenance_method": "similarity", "provenance_similarity_llm": path}, embeddings=emb)
        assert isinstance(a, DocumentSimilarityAttribution) and a.embeddings is emb and a.include_query is None
    with pytest.raises(KeyError):
        factory.provenance_from_env({"provenance_method": "similarity"}, embeddings=emb)
    with pytest.raises(FileNotFoundError):                           # the template's hub id: a local directory is required
        factory.provenance_from_env({"provenance_method": "similarity",
                                     "provenance_similarity_llm": "sentence-transformers/distiluse-base-multilingual-cased-v2"}, embeddings=emb)
    with pytest.raises(RuntimeError):
        factory.provenance_from_env({"provenance_method": "similarity", "provenance_similarity_llm": Spec.path, "force_cpu": "True"},
                                    embeddings=emb)
    # another directory: an embeddings object of its own over it
    from ragmeup_amd import embeddings as E
    built = []

    class Own:
        def __init__(self, model_dir=None, device=0):
            built.append((model_dir, device))

    monkeypatch.setattr(E, "MI355XEmbeddings", Own)
    other = tmp_path / "other"
    os.makedirs(other)
    for given in (emb, None):
        a = factory.provenance_from_env({"provenance_method": "similarity", "provenance_similarity_llm": str(other)}, embeddings=given)
        assert isinstance(a, DocumentSimilarityAttribution) and isinstance(a.embeddings, Own)
    assert built == [(str(other), 0)] * 2
