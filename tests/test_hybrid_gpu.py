"""GPU: the one-call hybrid (rmu_hybrid_search, rmu_bert_search_hybrid, MI355XHybridRetriever) against the calls it replaces: the members'
own searches fused by tests/rrf_ref.py through the same keys, and MI355XEnsembleRetriever over the same members."""
import numpy as np
import pytest

from tests.bm25_ref import synth_corpus, synth_queries
from tests.rrf_ref import fuse_arrays

pytestmark = pytest.mark.gpu


class _HashEmbeddings:
    """bag of words hashed into 64 dimensions (the store only needs vectors)"""

    def _one(self, t):
        v = np.zeros(64, np.float32)
        for w in t.split():
            v[sum(map(ord, w)) % 64] += 1.0
        return (v / max(np.linalg.norm(v), 1e-9)).tolist()

    def embed_documents(self, texts):
        return [self._one(t) for t in texts]

    def embed_query(self, text):
        return self._one(text)


def _corpus():
    """~400 texts with ~40 of them repeated at other positions, and a permutation: the sparse member holds the texts in another order"""
    rng = np.random.default_rng(77)
    texts = [t for t in synth_corpus(400, seed=77) if t]
    for i in rng.choice(len(texts), 40, replace=False).tolist():
        texts.insert(int(rng.integers(0, len(texts) + 1)), texts[i])
    perm = rng.permutation(len(texts)).tolist()
    return texts, [texts[p] for p in perm]


@pytest.fixture(scope="module")
def setup():
    from ragmeup_amd import FlatIndex
    from ragmeup_amd.bm25 import BM25Index
    from ragmeup_amd.hybrid import HybridIndex, content_keys
    texts, sparse_texts = _corpus()
    assert len(set(texts)) < len(texts) - 30 and texts != sparse_texts
    emb = _HashEmbeddings()
    bm25 = BM25Index()
    bm25.add_texts(sparse_texts)
    idx = FlatIndex(64)
    idx.add(np.asarray(emb.embed_documents(texts), np.float32))
    classes: dict = {}
    skeys, dkeys = content_keys(sparse_texts, classes), content_keys(texts, classes)
    h = HybridIndex(bm25, idx)
    h.set_keys(0, 0, skeys)
    h.set_keys(1, 0, dkeys)
    queries = synth_queries(texts, 64, seed=3)
    qv = np.asarray(emb.embed_documents(queries), np.float32)
    yield {"texts": texts, "sparse_texts": sparse_texts, "bm25": bm25, "idx": idx, "h": h, "skeys": skeys, "dkeys": dkeys, "queries": queries,
           "qv": qv, "emb": emb}
    h.close()
    idx.close()
    bm25.close()


def _expected(docs, rows, skeys, dkeys, weights, c=60, k_out=None):
    """the members' id lists -> what rmu_hybrid_search must return: (scores, ids, member)"""
    nq, ks = docs.shape
    kd = rows.shape[1]
    depth = max(ks, kd)
    k_out = ks + kd if k_out is None else k_out
    keys = np.full((2, nq, depth), -1, np.int64)
    if len(skeys):
        keys[0, :, :ks] = np.where(docs >= 0, skeys[np.maximum(docs, 0)], -1)
    if len(dkeys):
        keys[1, :, :kd] = np.where(rows >= 0, dkeys[np.maximum(rows, 0)], -1)
    s, _, src = fuse_arrays(keys, weights, c, k_out)
    member = np.where(src >= 0, src // depth, -1).astype(np.int32)
    pos = np.where(src >= 0, src % depth, 0)
    qi = np.arange(nq)[:, None]
    ids = np.where(member == 0, docs[qi, np.minimum(pos, ks - 1)], rows[qi, np.minimum(pos, kd - 1)])
    return s, np.where(member >= 0, ids, -1), member


def _same(got, want, what=None):
    assert np.array_equal(got[1], want[1]), what
    assert np.array_equal(got[2], want[2]), what
    assert np.array_equal(got[0].view(np.int64), want[0].view(np.int64)), what


@pytest.mark.parametrize("ks,fetch_k,kd", [(4, 20, 4), (5, 8, 8), (112, 64, 64)])
def test_one_call_equals_the_two_member_calls_fused(setup, ks, fetch_k, kd):
    s = setup
    seen_both = 0
    for nq in (1, 7, 64):
        queries, qv = s["queries"][:nq], s["qv"][:nq]
        _, docs = s["bm25"].search(queries, ks)
        for lam in (0.5, None):
            rows = s["idx"].search_mmr(qv, fetch_k, kd, lam)[0] if lam is not None else s["idx"].search(qv, kd)[1]
            for w in ((0.5, 0.5), (0.7, 0.3)):
                want = _expected(docs, rows, s["skeys"], s["dkeys"], w)
                got = s["h"].search(qv, queries, ks, fetch_k, kd, lam, w)
                _same(got, want, (nq, lam, w))
                seen_both += int(((got[2] == 0).any(axis=1) & (got[2] == 1).any(axis=1)).sum())
                # the keys carry the result: a hit's text is the same whichever member represents it, and no text comes back twice
                for q in range(nq):
                    hit = [s["sparse_texts"][i] if m == 0 else s["texts"][i] for i, m in zip(got[1][q], got[2][q]) if i >= 0]
                    assert len(hit) == len(set(hit))
    assert seen_both > 0
    # a k_out below the distinct count is the head of the full list
    got = s["h"].search(s["qv"][:7], s["queries"][:7], ks, fetch_k, kd, 0.5, (0.5, 0.5), k_out=3)
    full = s["h"].search(s["qv"][:7], s["queries"][:7], ks, fetch_k, kd, 0.5, (0.5, 0.5))
    _same(got, tuple(a[:, :3] for a in full))


def _pairs(hits):
    return [[(d.page_content, d.metadata) for d in h] for h in hits]


def test_the_retriever_returns_what_the_ensemble_returns(setup, monkeypatch):
    from ragmeup_amd._lc import Embeddings
    from ragmeup_amd.bm25 import MI355XBM25Retriever
    from ragmeup_amd.ensemble import MI355XEnsembleRetriever
    from ragmeup_amd.hybrid import HybridIndex, MI355XHybridRetriever
    from ragmeup_amd.vectorstore import MI355XVectorStore

    class HashEmbeddings(_HashEmbeddings, Embeddings):
        pass

    texts, sparse_texts = setup["texts"], setup["sparse_texts"]
    bm25 = MI355XBM25Retriever.from_texts(sparse_texts, metadatas=[{"doc": i, "source": f"f{i % 5}.pdf"} for i in range(len(sparse_texts))], k=5)
    store = MI355XVectorStore.from_texts(texts, HashEmbeddings(), metadatas=[{"row": i, "source": f"f{i % 5}.pdf"} for i in range(len(texts))],
                                         collection_name="hybrid-parity", auto_persist=False, drop_old=True)
    dense = store.as_retriever(search_type="mmr", search_kwargs={"k": 4, "fetch_k": 20})
    plain = store.as_retriever(search_kwargs={"k": 5})
    calls = []
    real = HybridIndex.search
    monkeypatch.setattr(HybridIndex, "search", lambda *a, **k: calls.append(1) or real(*a, **k))
    queries = setup["queries"][:12]
    hybrids = []

    def check(one_call=True):
        for d, w in ((dense, [0.5, 0.5]), (plain, [0.7, 0.3])):
            ens = MI355XEnsembleRetriever(retrievers=[bm25, d], weights=w)
            hyb = MI355XHybridRetriever(sparse=bm25, dense=d, weights=w)
            hybrids.append(hyb)
            del calls[:]
            assert _pairs(hyb.batch_invoke(queries)) == _pairs(ens.batch_invoke(queries))
            assert _pairs([hyb.invoke(q) for q in queries[:4]]) == _pairs([ens.invoke(q) for q in queries[:4]])
            assert len(calls) == (5 if one_call else 0)
        return hyb

    try:
        check()
        kept = MI355XHybridRetriever(sparse=bm25, dense=dense, weights=[0.5, 0.5])       # this one lives through every change below
        hybrids.append(kept)
        ens = MI355XEnsembleRetriever(retrievers=[bm25, dense], weights=[0.5, 0.5])

        def follow():
            assert _pairs(kept.batch_invoke(queries)) == _pairs(ens.batch_invoke(queries))
            assert _pairs([kept.invoke(queries[0])]) == _pairs([ens.invoke(queries[0])])
        follow()
        assert bm25.delete(expr='source == "f3.pdf"').delete_count > 0 and store.delete(expr='source == "f3.pdf"').delete_count > 0
        follow()
        check()
        assert bm25.compact() > 0 and store.compact() > 0
        follow()
        check()
        # records added to the members directly, one of them a text both already hold
        new = ["w1 w2 brand new text w3", texts[5], "another w7 w7 w9 text"]
        store.add_texts(new, metadatas=[{"row": 1000 + i, "source": "late.pdf"} for i in range(3)])
        bm25.add_texts(list(reversed(new)), [{"doc": 2000 + i, "source": "late.pdf"} for i in range(3)])
        del calls[:]
        follow()
        assert len(calls) == 2
        got = kept.invoke("brand new text another")
        assert _pairs([got]) == _pairs([ens.invoke("brand new text another")]) and any(d.metadata["source"] == "late.pdf" for d in got)
        check()
        # a filter on the members: the two-call fusion, same result
        flt = {"filter": {"source": "f1.pdf"}}
        bm25.search_kwargs = dict(flt)
        dense.search_kwargs = dict(dense.search_kwargs, **flt)
        plain.search_kwargs = dict(plain.search_kwargs, **flt)
        del calls[:]
        follow()
        assert not calls and all(d.metadata["source"] == "f1.pdf" for d in kept.invoke(queries[1]))
        check(one_call=False)
    finally:
        for hyb in hybrids:
            hyb.close()
        bm25.vectorizer.close()


def test_tables_out_of_step_are_refused_and_a_correct_search_still_works(setup):
    from ragmeup_amd import FlatIndex, _native
    from ragmeup_amd.hybrid import HybridIndex
    s = setup
    queries, qv = s["queries"][:7], s["qv"][:7]
    want = s["h"].search(qv, queries, 4, 20, 4)
    idx = FlatIndex(64)
    idx.add(np.asarray(s["emb"].embed_documents(s["texts"]), np.float32))
    h = HybridIndex(s["bm25"], idx)
    try:
        h.set_keys(0, 0, s["skeys"][:-1])
        h.set_keys(1, 0, s["dkeys"])
        with pytest.raises(_native.RmuError, match="out of step") as e:
            h.search(qv, queries, 4, 20, 4)
        assert e.value.code == -1 and "sparse" in str(e.value)
        h.set_keys(0, len(s["skeys"]) - 1, s["skeys"][-1:])               # the append that was missing
        _same(h.search(qv, queries, 4, 20, 4), want)
        idx.add(np.asarray(s["emb"].embed_documents(["w3 w4 w5"]), np.float32))  # a row the table does not know
        with pytest.raises(_native.RmuError, match="out of step") as e:
            h.search(qv, queries, 4, 20, 4)
        assert e.value.code == -1 and "dense" in str(e.value)
        h.set_keys(1, len(s["dkeys"]), [10 ** 6])
        got = h.search(qv, queries, 4, 20, 4)
        _, docs = s["bm25"].search(queries, 4)
        rows = idx.search_mmr(qv, 20, 4, 0.5)[0]
        _same(got, _expected(docs, rows, s["skeys"], np.append(s["dkeys"], 10 ** 6), (0.5, 0.5)))
        h.set_keys(1, 0, s["dkeys"][:5])                                  # a replacement that is too short
        with pytest.raises(_native.RmuError, match="out of step"):
            h.search(qv, queries, 4, 20, 4)
    finally:
        h.close()
        idx.close()


def test_a_member_with_nothing_live_leaves_the_other_members_list(setup):
    from ragmeup_amd import FlatIndex
    from ragmeup_amd.bm25 import BM25Index
    from ragmeup_amd.hybrid import HybridIndex
    s = setup
    queries, qv = s["queries"][:7], s["qv"][:7]
    w = (0.7, 0.3)
    gone = BM25Index()
    gone.add_texts(s["sparse_texts"])
    assert gone.remove(np.arange(len(s["sparse_texts"]))) == len(s["sparse_texts"])
    empty = FlatIndex(64)
    a, b = HybridIndex(gone, s["idx"]), HybridIndex(s["bm25"], empty)
    try:
        a.set_keys(0, 0, s["skeys"])
        a.set_keys(1, 0, s["dkeys"])
        rows = s["idx"].search_mmr(qv, 20, 4, 0.5)[0]
        got = a.search(qv, queries, 5, 20, 4, 0.5, w)
        _same(got, _expected(np.full((7, 5), -1, np.int64), rows, s["skeys"], s["dkeys"], w))
        assert np.all(got[2][got[1] >= 0] == 1) and np.all((got[1] >= 0).sum(axis=1) >= 3)
        assert got[0][0, 0] == 0.0 + 0.3 / 61
        b.set_keys(0, 0, s["skeys"])
        _, docs = s["bm25"].search(queries, 5)
        got = b.search(qv, queries, 5, 20, 4, 0.5, w)
        _same(got, _expected(docs, np.full((7, 4), -1, np.int64), s["skeys"], s["dkeys"][:0], w))
        assert np.all(got[2][got[1] >= 0] == 0) and np.all((got[1] >= 0).sum(axis=1) >= 1)
    finally:
        a.close()
        b.close()
        empty.close()
        gone.close()


def test_the_token_path_equals_the_fused_member_calls():
    """rmu_bert_search_hybrid against rmu_bert_search_mmr's rows and rmu_bm25_search's documents for the same token ids and texts"""
    from ragmeup_amd import FlatIndex
    from ragmeup_amd.bert import BertEncoder
    from ragmeup_amd.bm25 import BM25Index
    from ragmeup_amd.hybrid import HybridIndex, content_keys
    from tests.helpers import bert_weights_numpy, make_bert
    enc = BertEncoder(bert_weights_numpy(make_bert(seed=0, layers=6)), layers=6)
    texts, sparse_texts = _corpus()
    rng = np.random.default_rng(9)
    x = rng.standard_normal((len(texts), 384)).astype(np.float32)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    first = {}
    for i, t in enumerate(texts):                                          # equal texts hold equal vectors, as in a real store
        x[i] = x[first.setdefault(t, i)]
    idx = FlatIndex(384)
    idx.add(x)
    bm25 = BM25Index()
    bm25.add_texts(sparse_texts)
    classes: dict = {}
    skeys, dkeys = content_keys(sparse_texts, classes), content_keys(texts, classes)
    h = HybridIndex(bm25, idx)
    try:
        h.set_keys(0, 0, skeys)
        h.set_keys(1, 0, dkeys)
        for n, L in ((1, 12), (3, 30)):
            lens = rng.integers(4, L + 1, n).astype(np.int32)
            lens[0] = L
            ids = rng.integers(1000, 30522, (n, L)).astype(np.int32)
            ids[:, 0] = 101
            ids[np.arange(n), lens - 1] = 102
            queries = synth_queries(texts, n, seed=40 + n)
            _, docs = bm25.search(queries, 4)
            for lam in (0.5, None):
                for rep in range(3):                                       # eager, capture, replay
                    rows = enc.search_host(idx, ids, lens, 0, 20, 4, lam)[0]
                    got = h.search_tokens(enc, ids, lens, 0, queries, 4, 20, 4, lam, (0.5, 0.5))
                    _same(got, _expected(docs, rows, skeys, dkeys, (0.5, 0.5)), (n, L, lam, rep))
        other = HybridIndex(bm25, None)
        with pytest.raises(Exception, match="384"):
            other.search_tokens(enc, ids, lens, 0, queries, 4, 20, 4)
        other.close()
    finally:
        h.close()
        idx.close()
        bm25.close()
