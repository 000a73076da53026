"""GPU: rmu_bm25_search (bm25.hip: postings in HBM, fused score + top-k, finished by the scan's final merge) against the fp64 restatement of
the formula in tests/bm25_ref.py.  Small corpora reach many tiles per workgroup, many workgroups per query and the range boundaries through
the two testing switches (RMU_BM25_OPT_TILE_DOCS, RMU_BM25_OPT_MAX_WGS)."""
import numpy as np
import pytest

from tests.bm25_ref import BM25Ref, check_topk, synth_corpus, synth_queries

pytestmark = pytest.mark.gpu

KS = (1, 4, 10, 33, 112)
OPT_TILE, OPT_WGS = 1, 2


def _index(texts, tile=0, wgs=0, pieces=1, **params):
    from ragmeup_amd.bm25 import BM25Index
    ix = BM25Index(**params)
    step = -(-len(texts) // pieces) or 1
    for a in range(0, len(texts), step):
        ix.add_texts(texts[a:a + step])
    ix.set_option(OPT_TILE, tile)
    ix.set_option(OPT_WGS, wgs)
    return ix


_CORPORA: dict = {}


def _corpus(n):
    """(texts, reference), computed once per size and left unchanged"""
    if n not in _CORPORA:
        texts = ["a b", "a b c", "a"] if n == 3 else synth_corpus(n, seed=n)
        _CORPORA[n] = (texts, BM25Ref(texts))
    return _CORPORA[n]


def _query_set(texts, seed=5):
    """1, 2, 9 and 40 tokens, duplicated tokens, unknown tokens only, the empty query, unknown between known ones"""
    q = [synth_queries(texts, 1, seed + t, t, t)[0] for t in (1, 2, 9, 40)]
    w = (" ".join(texts).split() or ["w0"])
    q += [f"{w[0]} {w[-1]} {w[0]} {w[0]} {w[-1]}", "nowhere never", "", f"{w[len(w) // 2]} nowhere {w[0]}", "  \t "]
    return q


def _check_all(ix, ref, queries, ks=KS, **kw):
    for k in ks:
        s, d = ix.search(queries, k, **kw)
        assert s.shape == (len(queries), k) and s.dtype == np.float32 and d.dtype == np.int64
        for i, q in enumerate(queries):
            check_topk(ref, q, s[i], d[i], k, doc_base=kw.get("doc_base", 0))
    return s, d


@pytest.mark.parametrize("n,tile,wgs", [(1, 0, 0), (3, 0, 0), (70, 0, 0), (63, 64, 0), (64, 64, 0), (65, 64, 0), (64 * 5 + 1, 64, 0),
                                        (5000, 64, 1), (5000, 64, 3), (5000, 64, 64), (20000, 0, 0)])
def test_topk_against_the_fp64_formula(n, tile, wgs):
    texts, ref = _corpus(n)
    ix = _index(texts, tile, wgs)
    try:
        queries = _query_set(texts)
        if n == 3:
            queries += ["a", "c a", "b b c"]
        _check_all(ix, ref, queries)
        if n >= 64:          # the empty query: all scores are 0, the result is documents 0 .. k-1
            s, d = ix.search([""], 10)
            assert np.array_equal(d[0], np.arange(10)) and np.all(s == 0.0)
    finally:
        ix.close()


def test_negative_mean_idf_gives_negative_scores():
    """3 documents: idf(a), idf(b) < 0 < idf(c) and the mean is negative, so the replacement value is negative too"""
    texts, ref = _corpus(3)
    assert ref.idf["a"] < 0 and ref.idf["b"] < 0 and ref.idf["c"] > 0
    ix = _index(texts)
    try:
        s, d = ix.search(["a"], 4)
        assert np.all(s[0, :3] < 0) and d[0, 3] == -1 and np.isneginf(s[0, 3])
        check_topk(ref, "a", s[0], d[0], 4)
    finally:
        ix.close()


@pytest.mark.parametrize("n,tile,wgs", [(70, 0, 0), (5000, 64, 3)])
def test_a_term_in_every_document_takes_the_replaced_idf(n, tile, wgs):
    texts = synth_corpus(n, seed=100 + n, every="omni")
    ref = BM25Ref(texts)
    mean = np.mean([np.log(n - df + 0.5) - np.log(df + 0.5) for df in ref.df.values()])
    assert ref.df["omni"] == n and ref.idf["omni"] == pytest.approx(0.25 * mean) and ref.idf["omni"] > 0
    ix = _index(texts, tile, wgs)
    try:
        _check_all(ix, ref, ["omni", "omni w3 omni", "w1 omni w7 w0"] + _query_set(texts), ks=(1, 10, 112))
    finally:
        ix.close()


@pytest.mark.parametrize("nq", [1, 5, 130])
def test_batches(nq):
    texts, ref = _corpus(5000)
    ix = _index(texts, 64, 3)
    try:
        _check_all(ix, ref, synth_queries(texts, nq, seed=40 + nq), ks=(10,))
    finally:
        ix.close()


def test_caller_stream_and_doc_base():
    import torch
    texts, ref = _corpus(5000)
    ix = _index(texts)
    try:
        queries = synth_queries(texts, 5, seed=9)
        s0, d0 = ix.search(queries, 10)
        st = torch.cuda.Stream()
        s1, d1 = _check_all(ix, ref, queries, ks=(10,), stream=st.cuda_stream, doc_base=1 << 33)
        assert np.array_equal(s0.view(np.uint32), s1.view(np.uint32)) and np.array_equal(d0 + (1 << 33), d1)
    finally:
        ix.close()


def test_identical_documents_come_back_in_ascending_id_order():
    """20 copies of one text have identical (tf, dl), hence identical score bits; placed so that they straddle a tile boundary (64) and a
    workgroup-range boundary (3 workgroups over 5 tiles of 64: ranges of 2 tiles, i.e. a boundary at 128)"""
    base = synth_corpus(300, seed=77)
    copy = "tie alpha tie beta"
    for start in (54, 118):          # copies at [54, 74): across 64;  [118, 138): across 128
        texts = base[:start] + [copy] * 20 + base[start:]
        ref = BM25Ref(texts)
        for tile, wgs in ((64, 3), (64, 1), (0, 0)):
            ix = _index(texts, tile, wgs)
            try:
                for k in (20, 33, 7):
                    s, d = ix.search(["tie beta", "alpha"], k)
                    m = min(k, 20)
                    for i in range(2):
                        assert np.array_equal(d[i, :m], np.arange(start, start + m)), (start, tile, wgs, k, d[i])
                        assert len(set(s[i, :m].view(np.uint32).tolist())) == 1
                        check_topk(ref, ["tie beta", "alpha"][i], s[i], d[i], k)
            finally:
                ix.close()


def test_bits_do_not_depend_on_tile_grid_batch_or_add_pieces():
    texts, ref = _corpus(5000)
    batch = synth_queries(texts, 130, seed=21)
    k = 33

    def run(tile=0, wgs=0, pieces=1, queries=batch):
        ix = _index(texts, tile, wgs, pieces)
        try:
            s, d = ix.search(queries, k)
        finally:
            ix.close()
        return s.view(np.uint32), d

    s0, d0 = run()
    for i in (0, 64, 129):
        check_topk(ref, batch[i], s0[i].view(np.float32), d0[i], k)
    for tile, wgs in ((64, 0), (1024, 0), (0, 1), (0, 3), (64, 1), (64, 3), (1024, 3)):
        s, d = run(tile, wgs)
        assert np.array_equal(s, s0) and np.array_equal(d, d0), (tile, wgs)
    s, d = run(pieces=3)
    assert np.array_equal(s, s0) and np.array_equal(d, d0)
    for i in (0, 77, 129):               # a query alone versus inside the batch of 130
        s, d = run(queries=[batch[i]])
        assert np.array_equal(s[0], s0[i]) and np.array_equal(d[0], d0[i]), i
        s, d = run(64, 3, queries=[batch[i]])
        assert np.array_equal(s[0], s0[i]) and np.array_equal(d[0], d0[i]), i


def test_searches_follow_adds():
    """the image is rebuilt by the first search after an add; idf and avgdl change for the old documents too"""
    texts, _ = _corpus(5000)
    ix = _index(texts[:300], 64, 3)
    try:
        q = _query_set(texts[:300])
        _check_all(ix, BM25Ref(texts[:300]), q, ks=(10,))
        assert ix.add_texts(texts[300:1000]) == 300
        _check_all(ix, BM25Ref(texts[:1000]), q, ks=(10,))
    finally:
        ix.close()


def test_retriever_returns_the_documents_of_the_ids():
    from ragmeup_amd.bm25 import MI355XBM25Retriever
    texts, ref = _corpus(5000)
    metas = [{"row": i, "source": f"f{i % 7}.pdf"} for i in range(len(texts))]
    r = MI355XBM25Retriever.from_texts(texts, metadatas=metas)
    try:
        queries = synth_queries(texts, 6, seed=3)
        _, ids = r.vectorizer.search(queries, 4)
        per = r.batch_invoke(queries)
        for i, q in enumerate(queries):
            one = r.invoke(q)
            assert [d.metadata["row"] for d in one] == ids[i].tolist() == [d.metadata["row"] for d in per[i]]
            assert all(d.page_content == texts[d.metadata["row"]] and d.metadata == metas[d.metadata["row"]] for d in one)
        r.k = 7
        assert len(r.invoke(queries[0])) == 7
        r.k = 4
        r.add_texts(["zzunique term here"], [{"row": len(texts)}])
        assert r.invoke("zzunique")[0].metadata == {"row": len(texts)}
    finally:
        r.vectorizer.close()


def test_ensemble_of_bm25_and_dense_is_weighted_rrf_of_the_members():
    from ragmeup_amd.bm25 import MI355XBM25Retriever
    from ragmeup_amd.ensemble import MI355XEnsembleRetriever, weighted_reciprocal_rank
    from ragmeup_amd.vectorstore import MI355XVectorStore
    from ragmeup_amd._lc import Embeddings

    class HashEmbeddings(Embeddings):
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

    texts = [t for t in synth_corpus(400, seed=8) if t]
    texts = list(dict.fromkeys(texts))
    bm25 = MI355XBM25Retriever.from_texts(texts, k=5)
    store = MI355XVectorStore.from_texts(texts, HashEmbeddings(), collection_name="bm25-ensemble", auto_persist=False, drop_old=True)
    dense = store.as_retriever(search_kwargs={"k": 5})
    ens = MI355XEnsembleRetriever(retrievers=[bm25, dense], weights=[0.5, 0.5])
    queries = synth_queries(texts, 4, seed=2)
    try:
        batch = ens.batch_invoke(queries)
        for i, q in enumerate(queries):
            want = weighted_reciprocal_rank([bm25.invoke(q), dense.invoke(q)], [0.5, 0.5])
            for got in (ens.invoke(q), batch[i]):
                assert [d.page_content for d in got] == [d.page_content for d in want]
            assert 5 <= len(want) <= 10
    finally:
        bm25.vectorizer.close()
