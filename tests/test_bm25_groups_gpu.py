"""GPU: rmu_bm25_search_groups (bm25.hip: bm25_groups_kernel) -- one call against the per-list rmu_bm25_search_subset calls it replaces, bit
for bit, and against the fp64 formula over the live corpus restricted to each list (tests/bm25_live.check_subset: bm25_ref.check_topk's
three properties and its own bound, nothing new); through every state of the image; and through the three retrievers."""
import numpy as np
import pytest

from tests.bm25_groups import SIZES, assignment, case_lists, queries_of, removed_of, texts_of
from tests.bm25_live import OPT_TILE, OPT_WGS, LiveCorpus, check_subset, same_bits

pytestmark = pytest.mark.gpu

OPT_REPACK_ON_ADD = 8
KS = (4, 70, 112)
# (documents, tile, part cap): one tile + 1 document; 5 tiles + 1; many tiles under a cap that joins ranges; the default geometry
SHAPES = [(65, 64, 0), (321, 64, 0), (321, 64, 3), (5000, 64, 3), (5000, 64, 0), (5000, 0, 0)]


def _index(texts, tile=0, wgs=0, remove=None, repack_on_add=0):
    from ragmeup_amd.bm25 import BM25Index
    ix = BM25Index()
    ix.add_texts(texts)
    ix.set_option(OPT_TILE, tile)
    ix.set_option(OPT_WGS, wgs)
    ix.set_option(OPT_REPACK_ON_ADD, repack_on_add)
    if remove is not None and len(remove):
        ix.remove(remove)
    return ix


def _per_list(ix, queries, k, lists, ql, **kw):
    """the reference of the bits: one rmu_bm25_search_subset call per query, over its own list"""
    s = np.empty((len(queries), k), np.float32)
    d = np.empty((len(queries), k), np.int64)
    for i, q in enumerate(queries):
        s[i], d[i] = (x[0] for x in ix.search([q], k, docs=lists[ql[i]], **kw))
    return s, d


def _check(ix, corpus, queries, lists, ql, ks=KS, formula=True, **kw):
    for k in ks:
        got = ix.search_groups(queries, k, lists, ql, **kw)
        assert got[0].shape == (len(queries), k) and got[0].dtype == np.float32 and got[1].dtype == np.int64
        assert same_bits(got, _per_list(ix, queries, k, lists, ql, **kw)), k
        if formula:
            for i, q in enumerate(queries):
                check_subset(corpus, lists[ql[i]], q, got[0][i], got[1][i], k, doc_base=kw.get("doc_base", 0))


def _cases(n, removed, tile, nq=40):
    cases = case_lists(n, removed, tile or 64)
    names = list(cases)
    return [cases[name] for name in names], assignment(names, nq, seed=n)


@pytest.mark.parametrize("n,tile,wgs", SHAPES)
def test_one_call_equals_the_per_list_calls_and_the_formula(n, tile, wgs):
    texts, removed = texts_of(n), removed_of(n)
    corpus = LiveCorpus(texts)
    corpus.remove(removed)
    ix = _index(texts, tile, wgs, removed)
    try:
        lists, ql = _cases(n, removed, tile)
        _check(ix, corpus, queries_of(n, 40), lists, ql)
        # a single list, a single query, and lists that hold fewer candidates than k
        _check(ix, corpus, queries_of(n, 3)[:1], [lists[0]], [0], ks=(112,))
    finally:
        ix.close()


def test_every_document_live_and_more_lists_than_queries():
    n = 321
    texts = texts_of(n)
    corpus = LiveCorpus(texts)
    ix = _index(texts, 64, 0)
    try:
        lists, _ = _cases(n, None, 64)
        _check(ix, corpus, queries_of(n, 5), lists, [len(lists) - 2, 0, 3, 0, 1], ks=(4, 70))
    finally:
        ix.close()


@pytest.mark.parametrize("repack_on_add", [0, 1])
def test_through_the_image_life_cycle(repack_on_add):
    n = 321
    texts, removed = texts_of(n), removed_of(n)
    corpus = LiveCorpus(texts)
    ix = _index(texts, 64, 3, repack_on_add=repack_on_add)
    try:
        queries = queries_of(n, 12)
        lists, ql = _cases(n, removed, 64, nq=12)
        _check(ix, corpus, queries, lists, ql, ks=(4,))                        # packed, every document live
        before = ix.image_stat()
        more = texts_of(65)
        ix.add_texts(more)                                                     # grown: the grouped call splices (or repacks) first
        corpus.add(more)
        lists2, ql2 = _cases(n + 65, removed, 64, nq=12)
        _check(ix, corpus, queries, lists2, ql2, ks=(4, 70))
        after = ix.image_stat()
        assert (after["splices"] - before["splices"], after["packs"] - before["packs"]) == ((0, 1) if repack_on_add else (1, 0))
        ix.remove(removed)                                                     # stale: the grouped call refreshes first
        corpus.remove(removed)
        _check(ix, corpus, queries, lists2, ql2, ks=(4, 112))
        want = ix.search_groups(queries, 10, lists2, ql2)
        m = ix.compact()                                                       # dirty: renumbered, the lists mapped
        assert np.array_equal(m, corpus.compact())
        mapped = [m[x][m[x] >= 0] for x in lists2]
        got = ix.search_groups(queries, 10, mapped, ql2)
        assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32))
        assert np.array_equal(got[1], np.where(want[1] >= 0, m[np.maximum(want[1], 0)], -1))
        _check(ix, corpus, queries, mapped, ql2, ks=(4,))
    finally:
        ix.close()


def test_doc_base_and_a_callers_stream():
    import torch
    n = 5000
    texts, removed = texts_of(n), removed_of(n)
    corpus = LiveCorpus(texts)
    corpus.remove(removed)
    ix = _index(texts, 64, 3, removed)
    try:
        queries = queries_of(n, 8)
        lists, ql = _cases(n, removed, 64, nq=8)
        plain = ix.search_groups(queries, 10, lists, ql)
        _check(ix, corpus, queries, lists, ql, ks=(10,), doc_base=1 << 33)
        based = ix.search_groups(queries, 10, lists, ql, doc_base=1 << 33)
        assert np.array_equal(based[1], np.where(plain[1] >= 0, plain[1] + (1 << 33), -1))
        stream = torch.cuda.Stream()
        on_stream = ix.search_groups(queries, 10, lists, ql, stream=stream.cuda_stream)
        assert same_bits(on_stream, plain)
        assert stream.query()                                                  # drained on return
    finally:
        ix.close()


def test_bad_lists_are_refused_and_the_index_still_answers():
    from ragmeup_amd._native import RmuError
    n = 321
    texts = texts_of(n)
    ix = _index(texts, 64, 0)
    try:
        queries = queries_of(n, 4)
        good = [np.arange(10, 200), np.array([5, 300])]
        want = ix.search_groups(queries, 4, good, [0, 1, 1, 0])                # (the image is on the device from here on)
        for bad in (np.array([5, 4]), np.array([5, 5]), np.array([0, n]), np.array([-1, 3])):
            # used, or unused between two used lists (BM25Index.search_groups sends the range of lists a call uses): refused
            for lists, ql in (([good[0], bad], [0, 1, 1, 0]), ([good[0], bad, good[1]], [0, 2, 2, 0])):
                with pytest.raises(RmuError) as e:
                    ix.search_groups(queries, 4, lists, ql)
                assert e.value.code == -1 and "ascending" in str(e.value)
        assert same_bits(ix.search_groups(queries, 4, good, [0, 1, 1, 0]), want)
    finally:
        ix.close()


# ---- the retrievers ------------------------------------------------------------------------------------------------------------------------
class _Emb:
    """deterministic 384-d embeddings of a text: the dense member needs some, their values do not matter here"""

    def _vec(self, t):
        rng = np.random.default_rng(abs(hash(t)) % (1 << 32))
        v = rng.standard_normal(384).astype(np.float32)
        return (v / np.linalg.norm(v)).tolist()

    def embed_documents(self, texts):
        return [self._vec(t) for t in texts]

    def embed_query(self, text):
        return self._vec(text)


def _members(n=321, files=6):
    from ragmeup_amd.bm25 import MI355XBM25Retriever
    from ragmeup_amd.vectorstore import MI355XVectorStore
    texts = [f"{t} u{i}" for i, t in enumerate(texts_of(n))]                    # (distinct page_content: the fusion identifies documents by it)
    per = -(-n // files)
    metas = [{"source": f"f{i // per}.pdf", "row": i} for i in range(n)]        # an upload's chunks are appended together
    ids = [f"id-{i}" for i in range(n)]
    sparse = MI355XBM25Retriever.from_texts(texts, metadatas=metas, ids=ids, k=5)
    sparse.vectorizer.set_option(OPT_TILE, 64)
    store = MI355XVectorStore.from_texts(texts, _Emb(), metadatas=metas, ids=ids)
    return sparse, store, texts


def _same_docs(a, b):
    return [[d.page_content for d in row] for row in a] == [[d.page_content for d in row] for row in b]


def test_retrievers_with_per_request_filters_equal_the_per_request_calls():
    from ragmeup_amd.ensemble import MI355XEnsembleRetriever
    from ragmeup_amd.hybrid import MI355XHybridRetriever
    sparse, store, texts = _members()
    try:
        queries = queries_of(321, 12)
        srcs = ["f0.pdf", "f3.pdf", None, "f5.pdf", "f0.pdf", "nowhere.pdf", "f2.pdf", None, "f3.pdf", "f1.pdf", "f4.pdf", "f0.pdf"]
        exprs = [None if s is None else f'source == "{s}"' for s in srcs]
        sparse.delete(filter={"source": "f4.pdf"})                             # a deleted source never comes back
        store.delete(filter={"source": "f4.pdf"})
        sparse.delete(ids=[f"id-{i}" for i in range(0, 321, 9)])
        store.delete(ids=[f"id-{i}" for i in range(0, 321, 9)])

        def singly(make):
            out = []
            for q, e in zip(queries, exprs):
                r = make({} if e is None else {"expr": e})
                out.append(r.batch_invoke([q])[0])
            return out

        def sparse_with(kw):
            sparse.search_kwargs = kw
            return sparse

        def check_rows(rows):
            for s, row in zip(srcs, rows):
                assert all(d.metadata["source"] != "f4.pdf" and d.metadata["row"] % 9 for d in row)
                if s is not None:
                    assert all(d.metadata["source"] == s for d in row)
                if s in ("nowhere.pdf", "f4.pdf"):
                    assert row == []
                elif s is not None:
                    assert row

        want = singly(sparse_with)
        sparse.search_kwargs = {}
        assert len({e for e in exprs if e}) >= 2 and sparse._use_groups(sparse.vectorizer, [np.arange(3)] * 2)     # the grouped route is taken
        got = sparse.batch_invoke(queries, exprs=exprs)
        assert _same_docs(got, want)
        check_rows(got)
        assert _same_docs(sparse.batch_invoke(queries, filters=[None if s is None else {"source": s} for s in srcs]), want)

        dense_kw = {"k": 4, "fetch_k": 12}
        for cls in (MI355XEnsembleRetriever, MI355XHybridRetriever):
            def make(kw, cls=cls):
                sparse.search_kwargs = kw
                dense = store.as_retriever(search_type="mmr", search_kwargs={**dense_kw, **kw})
                return (cls(retrievers=[sparse, dense], weights=[0.5, 0.5]) if cls is MI355XEnsembleRetriever
                        else cls(sparse=sparse, dense=dense, weights=[0.5, 0.5]))
            want = singly(make)
            got = make({}).batch_invoke(queries, exprs=exprs)
            assert _same_docs(got, want), cls.__name__
            check_rows(got)
    finally:
        sparse.vectorizer.close()
