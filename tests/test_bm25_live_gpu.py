"""GPU: BM25 searches over an index with removed documents and over a subset of its documents (bm25.hip: bm25_masked_kernel; include/rmu.h,
"Live documents") against the fp64 formula over the LIVE texts (tests/bm25_live.py), and bit for bit across the paths that must agree:
refresh against repack, every tile and grid, alone against in a batch, before against after a compact, saved against loaded."""
import numpy as np
import pytest

from tests.bm25_live import OPT_REPACK, OPT_TILE, OPT_WGS, LiveCorpus, check_all, check_live, same_bits
from tests.bm25_ref import BM25Ref, synth_corpus, synth_queries
from tests.test_bm25_gpu import _query_set

pytestmark = pytest.mark.gpu

KS = (1, 10, 33, 112)
SHAPES = [(65, 64, 0), (64 * 5 + 1, 64, 0), (5000, 64, 3), (5000, 0, 0), (20000, 0, 0)]
_TEXTS: dict = {}


def _texts(n, **kw):
    key = (n, tuple(sorted(kw.items())))
    if key not in _TEXTS:
        _TEXTS[key] = synth_corpus(n, seed=n, **kw)
    return _TEXTS[key]


def _index(texts, tile=0, wgs=0, repack=0, **params):
    from ragmeup_amd.bm25 import BM25Index
    ix = BM25Index(**params)
    ix.add_texts(texts)
    ix.set_option(OPT_TILE, tile)
    ix.set_option(OPT_WGS, wgs)
    ix.set_option(OPT_REPACK, repack)
    return ix


def _wg_range(n, tile, wgs, nq):
    """the documents of the second workgroup of a query (the library's geometry, restated: bm25.hip, "geometry")"""
    if not tile:
        tile = 8192
        while tile > 1024 and -(-n // tile) * nq < 1024:
            tile >>= 1
    tiles = -(-n // tile)
    per_wg = -(-tiles // (wgs or min(1024, max(8, 4096 // nq))))
    assert -(-tiles // per_wg) >= 2
    return np.arange(per_wg * tile, min(2 * per_wg * tile, n))


def _pattern(name, n, tile, wgs, ix, queries):
    if name == "ends":
        return [0, n - 1]
    if name == "word_and_tile_edges":
        return [31, 32, 63, 64]
    if name == "one_tile":
        return np.arange(64, min(128, n))
    if name == "one_workgroup_range":
        return _wg_range(n, tile, wgs, len(queries))
    if name == "every_second":
        return np.arange(0, n, 2)
    if name == "all_but_one":
        return np.delete(np.arange(n), n // 2)
    if name == "top1_of_each_query":
        _, d = ix.search(queries, 1)
        return np.unique(d[d >= 0])
    if name == "fewer_live_than_k":
        return np.delete(np.arange(n), [0, 63, 64, n // 2, n - 1])
    raise AssertionError(name)


PATTERNS = ["ends", "word_and_tile_edges", "one_tile", "one_workgroup_range", "every_second", "all_but_one", "top1_of_each_query",
            "fewer_live_than_k"]


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("n,tile,wgs", SHAPES)
def test_removed_documents_against_the_fp64_formula_over_the_live_corpus(n, tile, wgs, pattern):
    texts = _texts(n)
    c = LiveCorpus(texts)
    queries = _query_set(texts)
    ix = _index(texts, tile, wgs)
    try:
        ids = _pattern(pattern, n, tile, wgs, ix, queries)
        assert ix.remove(ids) == c.remove(ids) == len(ids)
        check_all(ix, c, queries, KS)
        # the empty query: every live document scores 0, the result is the first k live ids
        s, d = ix.search([""], 10)
        m = min(10, len(c.live_ids))
        assert np.array_equal(d[0, :m], c.live_ids[:m]) and np.all(s[0, :m] == 0.0) and np.all(d[0, m:] == -1)
    finally:
        ix.close()


@pytest.mark.parametrize("n,tile,wgs", [(321, 64, 0), (5000, 64, 3)])
def test_a_word_whose_documents_are_all_removed_is_an_unknown_word(n, tile, wgs):
    texts = _texts(n)
    c = LiveCorpus(texts)
    word = "w9"
    holders = [i for i, t in enumerate(texts) if word in t.split()]
    assert 0 < len(holders) < n // 2
    ix = _index(texts, tile, wgs)
    try:
        ix.search([word], 4)                                           # a clean image first: the removal takes the refresh path
        assert ix.remove(holders) == c.remove(holders)
        assert ix.df(word) == 0 and word not in c.ref.df
        queries = [word, f"w1 {word} w3", f"{word} {word}"] + _query_set(texts)
        check_all(ix, c, queries, KS)
        a = ix.search([f"w1 {word} w3", word], 33)
        b = ix.search(["w1 nowhere w3", "nowhere"], 33)
        assert same_bits(a, b)
    finally:
        ix.close()


def _raw_idf(ref, term):
    return float(np.log(ref.n - ref.df[term] + 0.5) - np.log(ref.df[term] + 0.5))


@pytest.mark.parametrize("n,tile,wgs", [(321, 64, 0), (5000, 64, 3)])
def test_removals_change_which_idf_is_replaced(n, tile, wgs):
    """"omni" is in every document (its idf is always the replacement); a word of fewer than half the documents has a positive idf until
    enough documents without it are removed -- then it takes the replacement too, and the mean the replacement is made of has moved"""
    texts = _texts(n, every="omni")
    c = LiveCorpus(texts)
    full = BM25Ref(texts)
    word = next(w for w in (f"w{i}" for i in range(3, 40)) if 0.25 * n < full.df[w] < 0.45 * n)
    assert _raw_idf(full, word) > 0 and _raw_idf(full, "omni") < 0
    without = [i for i, t in enumerate(texts) if word not in t.split()]
    ids = without[:int(0.7 * len(without))]
    ix = _index(texts, tile, wgs)
    try:
        queries = ["omni", word, f"{word} omni w1", "w1 omni w7 w0"] + _query_set(texts)
        check_all(ix, c, queries, (10,))
        assert ix.remove(ids) == c.remove(ids)
        ref = c.ref
        assert _raw_idf(ref, word) < 0 and ref.idf[word] == ref.idf["omni"] > 0 and ref.idf["omni"] != full.idf["omni"]
        check_all(ix, c, queries, KS)
    finally:
        ix.close()


def _removal(n):
    """a block across a tile boundary, a stride, the ends"""
    return np.unique(np.concatenate([np.arange(40, 200), np.arange(0, n, 7), [n - 1]]))


def test_bits_do_not_depend_on_the_path_the_tile_the_grid_or_the_batch():
    texts = _texts(5000)
    c = LiveCorpus(texts)
    ids = _removal(5000)
    c.remove(ids)
    batch = synth_queries(texts, 130, seed=21)
    k = 33

    def run(tile=0, wgs=0, repack=0, queries=batch, warm=True):
        ix = _index(texts, tile, wgs, repack)
        try:
            if warm:
                ix.search(queries[:1], k)              # the image is clean when the documents go: refresh path (repack = 0)
            ix.remove(ids)
            return ix.search(queries, k)
        finally:
            ix.close()

    base = run()
    for i in (0, 64, 129):
        check_live(c, batch[i], base[0][i], base[1][i], k)
    assert same_bits(run(repack=1), base)                                # refresh against repack
    assert same_bits(run(warm=False), base)                              # removed before the first image: packed without them
    for tile, wgs in ((64, 0), (1024, 0), (0, 1), (64, 3)):
        assert same_bits(run(tile, wgs), base), (tile, wgs)
        assert same_bits(run(tile, wgs, repack=1), base), (tile, wgs)
    for i in (0, 77, 129):                                               # a query alone against inside the batch of 130
        for tile, wgs in ((0, 0), (64, 3)):
            s, d = run(tile, wgs, queries=[batch[i]])
            assert same_bits((s[0], d[0]), (base[0][i], base[1][i])), (i, tile, wgs)


def test_bits_survive_compact_save_and_load(tmp_path):
    from ragmeup_amd.bm25 import BM25Index
    texts = _texts(5000)
    ids = _removal(5000)
    queries = synth_queries(texts, 20, seed=33) + _query_set(texts)
    k = 33
    ix = _index(texts, 64, 3)
    try:
        ix.search(queries[:1], k)
        ix.remove(ids)
        before = ix.search(queries, k)
        path = str(tmp_path / "ix.bm25")
        ix.save(path)                                                    # with the removed documents in it
        back = BM25Index.load(path)
        try:
            assert back.stat() == ix.stat()
            assert same_bits(back.search(queries, k), before)
            back.set_option(OPT_TILE, 64)
            assert same_bits(back.search(queries, k), before)
        finally:
            back.close()
        m = ix.compact()
        assert (m >= 0).sum() == 5000 - len(ids) and len(ix) == 5000 - len(ids)
        s, d = ix.search(queries, k)
        new_of_old = np.where(before[1] >= 0, m[np.maximum(before[1], 0)], -1)
        assert np.all(new_of_old[before[1] >= 0] >= 0)
        assert same_bits((s, d), (before[0], new_of_old))
        ix.save(path)                                                    # compacted: a term may be left without postings
        back = BM25Index.load(path)
        try:
            assert same_bits(back.search(queries, k), (s, d))
        finally:
            back.close()
    finally:
        ix.close()


def test_remove_add_search_equals_the_repacking_handle():
    texts = _texts(5000)
    queries = synth_queries(texts, 10, seed=5) + _query_set(texts)

    def run(repack):
        ix = _index(texts[:3000], 64, 3, repack)
        try:
            out = [ix.search(queries, 10)]
            ix.remove(_removal(3000))
            out.append(ix.search(queries, 10))
            ix.remove([1, 2, 3])
            assert ix.add_texts(texts[3000:]) == 3000              # the add makes the image dirty on either handle
            out.append(ix.search(queries, 10))
            ix.remove(np.arange(2990, 3100))
            out.append(ix.search(queries, 112))
            return out
        finally:
            ix.close()

    for a, b in zip(run(0), run(1)):
        assert same_bits(a, b)


def test_searches_follow_removals_adds_and_compacts():
    texts = _texts(5000)
    c = LiveCorpus(texts[:700])
    ix = _index(texts[:700], 64, 3)
    try:
        q = _query_set(texts[:700])
        check_all(ix, c, q, (10,))
        assert ix.remove(np.arange(100, 300)) == c.remove(np.arange(100, 300))
        check_all(ix, c, q, (10, 112))
        assert ix.add_texts(texts[700:1500]) == 700
        c.add(texts[700:1500])
        check_all(ix, c, q, (10,))
        assert ix.remove([0, 699, 700, 1499, 150]) == c.remove([0, 699, 700, 1499, 150]) == 4
        check_all(ix, c, q, (10,))
        assert np.array_equal(ix.compact(), c.compact()) and len(ix) == len(c.texts) == 1296
        check_all(ix, c, q, (10, 112))
        assert ix.remove([5]) == c.remove([5])
        assert ix.add_texts(texts[1500:1600]) == 1296
        c.add(texts[1500:1600])
        check_all(ix, c, q, (10,))
    finally:
        ix.close()


# ---- subset --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,tile", [(65, 64), (112, 0), (100, 64)])
def test_a_filtered_topk_is_the_unfiltered_ranking_restricted_to_the_list(n, tile):
    texts = _texts(n)
    queries = _query_set(texts)
    ix = _index(texts, tile)
    try:
        full_s, full_d = ix.search(queries, n)
        for allow in (np.arange(n), np.arange(1, n, 3), np.array([0, 31, 32, 63, 64]), np.array([n - 1]), np.arange(60, n)):
            for k in (1, 10, min(n, 112)):
                s, d = ix.search(queries, k, docs=allow)
                for i in range(len(queries)):
                    keep = np.isin(full_d[i], allow)
                    m = min(k, int(keep.sum()))
                    assert np.array_equal(d[i, :m], full_d[i][keep][:m]) and np.all(d[i, m:] == -1), (allow, k, i)
                    assert np.array_equal(s[i, :m].view(np.uint32), full_s[i][keep][:m].view(np.uint32)) and np.all(np.isneginf(s[i, m:]))
    finally:
        ix.close()


def test_subsets_of_5000_documents():
    texts = _texts(5000)
    c = LiveCorpus(texts)
    queries = _query_set(texts)
    ix = _index(texts, 64, 3)
    try:
        rng = np.random.default_rng(3)
        lists = [np.array([4321]), np.sort(rng.choice(5000, 33, replace=False)), np.arange(1728, 1792), np.arange(0, 5000, 7),
                 np.arange(5000), np.zeros(0, np.int64)]
        for allow in lists:
            check_all(ix, c, queries, KS, allow=allow)
        # a list combined with removals: the candidates are the list's live documents, the statistics the live corpus's
        ids = _removal(5000)
        assert ix.remove(ids) == c.remove(ids)
        for allow in (np.arange(0, 5000, 7), np.arange(30, 260), np.arange(5000), np.sort(rng.choice(5000, 33, replace=False))):
            check_all(ix, c, queries, (10, 112), allow=allow)
        s, d = ix.search(queries, 10, docs=np.arange(0, 5000, 7))       # every one of them removed
        assert np.all(d == -1) and np.all(np.isneginf(s))
        # the scores are those of the unfiltered search
        full = ix.search(queries[:4], 112)
        allow = np.arange(1, 5000, 2)
        sub = ix.search(queries[:4], 20, docs=allow)
        for i in range(4):
            keep = np.isin(full[1][i], allow)
            assert same_bits((sub[0][i], sub[1][i]), (full[0][i][keep][:20], full[1][i][keep][:20]))
    finally:
        ix.close()


def test_subset_with_a_caller_stream_and_doc_base():
    import torch
    texts = _texts(5000)
    c = LiveCorpus(texts)
    ix = _index(texts)
    try:
        ids = _removal(5000)
        assert ix.remove(ids) == c.remove(ids)
        queries = synth_queries(texts, 5, seed=9)
        allow = np.arange(3, 5000, 5)
        a = ix.search(queries, 10, docs=allow)
        st = torch.cuda.Stream()
        b = check_all(ix, c, queries, (10,), allow=allow, stream=st.cuda_stream, doc_base=1 << 33)
        assert same_bits(a, (b[0], b[1] - (1 << 33)))
        b = check_all(ix, c, queries, (10,), stream=st.cuda_stream, doc_base=1 << 33)
        assert same_bits(ix.search(queries, 10), (b[0], b[1] - (1 << 33)))
    finally:
        ix.close()


# ---- retriever and ensemble ------------------------------------------------------------------------------------------------------------
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


def _members(name, sparse_kw=None, dense_kw=None):
    from ragmeup_amd._lc import Embeddings
    from ragmeup_amd.bm25 import MI355XBM25Retriever
    from ragmeup_amd.vectorstore import MI355XVectorStore

    class HashEmbeddings(_HashEmbeddings, Embeddings):
        pass

    texts = list(dict.fromkeys(t for t in synth_corpus(400, seed=8) if t))
    metas = [{"row": i, "source": f"f{i % 5}.pdf"} for i in range(len(texts))]
    bm25 = MI355XBM25Retriever.from_texts(texts, metadatas=metas, k=5, **(sparse_kw or {}))
    store = MI355XVectorStore.from_texts(texts, HashEmbeddings(), metadatas=metas, collection_name=name, auto_persist=False, drop_old=True)
    dense = store.as_retriever(search_kwargs=dict({"k": 5}, **(dense_kw or {})))
    return texts, bm25, store, dense


def test_a_deleted_source_never_comes_back():
    from ragmeup_amd.ensemble import MI355XEnsembleRetriever
    texts, bm25, store, dense = _members("bm25-live-delete")
    ens = MI355XEnsembleRetriever(retrievers=[bm25, dense], weights=[0.5, 0.5])
    queries = synth_queries(texts, 6, seed=2)
    try:
        assert any(d.metadata["source"] == "f3.pdf" for q in queries for d in bm25.invoke(q))
        n = sum(1 for i in range(len(texts)) if i % 5 == 3)
        assert bm25.delete(expr='source == "f3.pdf"').delete_count == n == store.delete(expr='source == "f3.pdf"').delete_count
        hits = [bm25.invoke(q) for q in queries] + bm25.batch_invoke(queries) + [ens.invoke(q) for q in queries] + ens.batch_invoke(queries)
        assert all(len(h) >= 5 for h in hits)
        assert all(d.metadata["source"] != "f3.pdf" for h in hits for d in h)
        # the documents that do come back are those of their ids
        _, ids = bm25.vectorizer.search(queries, 5)
        assert [[d.metadata["row"] for d in h] for h in bm25.batch_invoke(queries)] == ids.tolist()
        # and after a compact the same documents, renumbered
        want = [[d.page_content for d in h] for h in bm25.batch_invoke(queries)]
        assert bm25.compact() == n and len(bm25.docs) == len(texts) - n
        assert [[d.page_content for d in h] for h in bm25.batch_invoke(queries)] == want
    finally:
        bm25.vectorizer.close()


def test_a_filter_on_both_members_restricts_every_fused_hit():
    from ragmeup_amd.ensemble import MI355XEnsembleRetriever
    kw = {"filter": {"source": "f1.pdf"}}
    texts, bm25, store, dense = _members("bm25-live-filter", {"search_kwargs": kw}, kw)
    ens = MI355XEnsembleRetriever(retrievers=[bm25, dense], weights=[0.5, 0.5])
    queries = synth_queries(texts, 6, seed=4)
    try:
        hits = [ens.invoke(q) for q in queries] + ens.batch_invoke(queries) + bm25.batch_invoke(queries) + [bm25.invoke(queries[0])]
        assert all(len(h) >= 5 for h in hits)
        assert all(d.metadata["source"] == "f1.pdf" for h in hits for d in h)
        bm25.search_kwargs = {"expr": 'source == "f2.pdf"'}
        assert all(d.metadata["source"] == "f2.pdf" for h in bm25.batch_invoke(queries) for d in h)
    finally:
        bm25.vectorizer.close()
