"""GPU: rmu_index_search_subset -- exact top-k over the rows one ascending list names (the gathered scan of scan_subset.hip) -- against the
fp64 oracle run on x[rows], bit for bit against the unfiltered search, under tombstones and compaction, with ties, device inputs on a
caller stream, and through the vector store's `filter=` / `expr=` on every search entry point.

Tolerance and tie rule are the project's own (tests/helpers.assert_topk_parity: ids identical, swaps only between fp64 scores within 1e-6,
scores within 1e-4); the oracle is oracle.flat_search(q, x[rows], k + 8, metric) with the returned positions mapped through `rows`."""
import hashlib

import numpy as np
import pytest

from oracle import oracle as O
from tests.helpers import assert_topk_parity

pytestmark = pytest.mark.gpu

N_ROWS = 20_011          # not a multiple of any tile


@pytest.fixture(scope="module")
def rmu():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import ragmeup_amd
    from ragmeup_amd import _native
    _native.lib()
    return ragmeup_amd


def _metric(name):
    from ragmeup_amd import _native as N
    return {"ip": N.METRIC_IP, "cosine": N.METRIC_COSINE, "l2": N.METRIC_L2SQ}[name]


def _corpus(metric, dim, n=N_ROWS):
    x = O.make_corpus(n, dim, seed=1000 + dim)
    q, _ = O.make_queries(x, 200, seed=77 + dim)
    if metric != "ip":       # rows of different length: the cosine normalisation / the L2 norm column matter
        x = (x * np.random.default_rng(5).uniform(0.5, 1.5, (n, 1))).astype(np.float32)
    return x, q


def _subsets(n, seed=11):
    rng = np.random.default_rng(seed)
    pick = lambda m: np.sort(rng.choice(n, m, replace=False)).astype(np.int64)
    return {
        "random 1%": pick(n // 100),
        "random 50%": pick(n // 2),
        "contiguous block": np.arange(5_003, 9_001, dtype=np.int64),
        "every 128th row": np.arange(0, n, 128, dtype=np.int64),
        "not a tile multiple": pick(1_037),
        "shorter than k": pick(5),
        "empty": np.zeros(0, np.int64),
    }


def _oracle(q, x, rows, k, metric):
    os_, op = O.flat_search(q, x[rows], k + 8, metric=metric)
    return os_, np.where(op >= 0, rows[np.maximum(op, 0)] if rows.size else -1, -1)


def _check(s, r, q, x, rows, k, metric, what):
    from ragmeup_amd import _native as N
    os_, or_ = _oracle(q, x, rows, k, metric)
    try:
        assert_topk_parity(-s if metric == N.METRIC_L2SQ else s, r, os_, or_)
    except AssertionError as e:
        raise AssertionError(f"{what}: {e}") from None
    live = r[r >= 0]
    assert np.isin(live, rows).all(), what
    want = min(k, rows.size)
    assert ((r >= 0).sum(1) == want).all(), what


_INDEXES = {}


def _index(rmu, metric, dim):
    key = (metric, dim)
    if key not in _INDEXES:
        _INDEXES.clear()                 # one index at a time in HBM
        x, q = _corpus(metric, dim)
        idx = rmu.FlatIndex(dim, metric=_metric(metric))
        idx.add(x[:7_000]); idx.add(x[7_000:])
        _INDEXES[key] = (idx, x, q)
    return _INDEXES[key]


CASES = [(m, d) for m in ("ip", "cosine") for d in (64, 384, 768)] + [("l2", d) for d in (64, 384, 700)]


@pytest.mark.parametrize("nq", [1, 7, 33, 200])
@pytest.mark.parametrize("metric,dim", CASES)
def test_parity_with_the_fp64_oracle(rmu, metric, dim, nq):
    idx, x, q = _index(rmu, metric, dim)
    for name, rows in _subsets(x.shape[0]).items():
        for k in (1, 10, 112):
            s, r = idx.search(q[:nq], k, rows=rows)
            assert s.shape == (nq, k) and r.shape == (nq, k)
            _check(s, r, q[:nq], x, rows, k, _metric(metric), f"{metric} d={dim} nq={nq} k={k} subset={name}")


@pytest.mark.parametrize("screening", [True, False])
@pytest.mark.parametrize("metric", ["ip", "cosine", "l2"])
def test_the_full_list_is_the_unfiltered_search_bit_for_bit(rmu, metric, screening):
    x, q = _corpus(metric, 384)
    idx = rmu.FlatIndex(384, metric=_metric(metric))
    idx.add(x)
    if screening:
        idx.set_screen_min_batch(1)      # the fp16 screening path + exact re-score, whatever the corpus size
    else:
        idx.set_screening(False)
    n = x.shape[0]
    every = np.arange(n, dtype=np.int64)
    some = np.sort(np.random.default_rng(2).choice(n, n // 3, replace=False)).astype(np.int64)
    for nq in (1, 40, 200):
        for k in (10, 100, 112):
            s0, r0 = idx.search(q[:nq], k)
            if screening and k <= 100:
                assert idx.last_screened() != 0
            s1, r1 = idx.search(q[:nq], k, rows=every)
            assert np.array_equal(r1, r0), (metric, nq, k)
            assert np.array_equal(s1.view(np.int32), s0.view(np.int32)), (metric, nq, k)
        # a random subset: every (row, score) it returns that the unfiltered top-112 also holds has the same score bits
        s0, r0 = idx.search(q[:nq], 112)
        s2, r2 = idx.search(q[:nq], 112, rows=some)
        shared = 0
        for qi in range(nq):
            full = dict(zip(r0[qi].tolist(), s0[qi].view(np.int32).tolist()))
            for row, bits in zip(r2[qi].tolist(), s2[qi].view(np.int32).tolist()):
                if row in full:
                    shared += 1
                    assert full[row] == bits, (metric, nq, qi, row)
        assert shared > 10 * nq


@pytest.mark.parametrize("metric", ["ip", "l2"])
def test_tombstoned_rows_never_appear_and_compaction_maps_the_list(rmu, metric):
    x, q = _corpus(metric, 384)
    n = x.shape[0]
    idx = rmu.FlatIndex(384, metric=_metric(metric))
    idx.add(x)
    rng = np.random.default_rng(9)
    rows = np.sort(rng.choice(n, 4_000, replace=False)).astype(np.int64)
    dead = np.sort(np.concatenate([rng.choice(rows, 1_500, replace=False), rng.choice(n, 3_000, replace=False)]))
    dead = np.unique(dead).astype(np.int64)
    idx.remove_rows(dead)
    alive_rows = rows[~np.isin(rows, dead)]
    before = {}
    for nq, k in ((1, 10), (50, 112)):
        s, r = idx.search(q[:nq], k, rows=rows)          # the list still names the dead rows
        assert not np.isin(r[r >= 0], dead).any()
        _check(s, r, q[:nq], x, alive_rows, k, _metric(metric), f"tombstones {metric} nq={nq} k={k}")
        before[(nq, k)] = (s, r)
    m = idx.compact()
    new_rows = m[rows]
    new_rows = new_rows[new_rows >= 0]
    assert new_rows.size == alive_rows.size and (np.diff(new_rows) > 0).all()
    for (nq, k), (s, r) in before.items():
        s2, r2 = idx.search(q[:nq], k, rows=new_rows)
        assert np.array_equal(r2, np.where(r >= 0, m[np.maximum(r, 0)], -1))
        assert np.array_equal(s2.view(np.int32), s.view(np.int32))


def test_equal_scores_come_back_lowest_row_first(rmu):
    x, q = _corpus("ip", 384, n=6_000)
    x = x.copy()
    dup = [7, 100, 2_047, 2_048, 5_000]
    for r in dup:
        x[r] = x[3]
    idx = rmu.FlatIndex(384, metric=_metric("ip"))
    idx.add(x)
    rows = np.unique(np.concatenate([np.arange(0, 6_000, 3), np.array(dup)])).astype(np.int64)      # holds row 3 and every duplicate
    qq = np.stack([x[3]] + [q[i] for i in range(39)])
    for nq in (1, 40):
        for k in (4, 10, 64):
            s, r = idx.search(qq[:nq], k, rows=rows)
            want, m = sorted([3] + dup), min(6, k)
            assert r[0, :m].tolist() == want[:m], (nq, k, r[0])
            assert (s[0, :m].view(np.int32) == s[0, :1].view(np.int32)).all()
            _check(s, r, qq[:nq], x, rows, k, _metric("ip"), f"ties nq={nq} k={k}")


def test_device_inputs_on_a_caller_stream_and_row_base(rmu):
    import torch
    x, q = _corpus("cosine", 384)
    idx = rmu.FlatIndex(384, metric=_metric("cosine"))
    idx.add(x)
    rows = _subsets(x.shape[0])["random 50%"]
    k, nq = 10, 64
    s_host, r_host = idx.search(q[:nq], k, rows=rows)
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        qd = torch.from_numpy(q[:nq]).cuda()
        rd = torch.from_numpy(rows).cuda()
        out = (torch.empty((nq, k), dtype=torch.float32, device="cuda"), torch.empty((nq, k), dtype=torch.int64, device="cuda"))
        st.synchronize()
        os_, or_ = idx.search(qd, k, row_base=1_000_000, stream=st.cuda_stream, out=out, rows=rd)
        assert os_ is out[0] and or_ is out[1]
        st.synchronize()
    assert np.array_equal(or_.cpu().numpy(), r_host + 1_000_000)
    assert np.array_equal(os_.cpu().numpy().view(np.int32), s_host.view(np.int32))
    # a device list may name ids outside the index: they are ignored
    wild = torch.cat([rd, torch.tensor([x.shape[0], x.shape[0] + 5, 2 ** 31 + 7, 2 ** 40], dtype=torch.int64, device="cuda")])
    s3, r3 = idx.search(qd, k, rows=wild)
    torch.cuda.synchronize()
    assert np.array_equal(r3.cpu().numpy(), r_host)
    # host list, row_base
    s4, r4 = idx.search(q[:nq], k, row_base=77, rows=rows)
    assert np.array_equal(r4, r_host + 77) and np.array_equal(s4.view(np.int32), s_host.view(np.int32))


def test_more_queries_than_one_launch_takes(rmu):
    n, d, k = 3_000, 64, 5
    x = O.make_corpus(n, d, seed=21)
    rng = np.random.default_rng(22)
    q = rng.standard_normal((8192 + 5, d)).astype(np.float32)
    idx = rmu.FlatIndex(d, metric=_metric("ip"))
    idx.add(x)
    rows = np.sort(rng.choice(n, n // 2, replace=False)).astype(np.int64)
    s, r = idx.search(q, k, rows=rows)
    _check(s, r, q, x, rows, k, _metric("ip"), "8192 + 5 queries")


def test_host_lists_are_validated_before_anything_runs(rmu):
    from ragmeup_amd import _native as N
    x, q = _corpus("ip", 64, n=2_000)
    idx = rmu.FlatIndex(64, metric=_metric("ip"))
    idx.add(x)
    good = np.arange(10, 500, 7, dtype=np.int64)
    s0, r0 = idx.search(q[:3], 5, rows=good)
    for bad in (good[::-1].copy(), np.array([1, 2, 2, 3], np.int64), np.array([-1, 4, 9], np.int64), np.array([5, 1_999, 2_000], np.int64)):
        with pytest.raises(N.RmuError) as e:
            idx.search(q[:3], 5, rows=bad)
        assert e.value.code == -1                      # RMU_E_INVALID
        s1, r1 = idx.search(q[:3], 5, rows=good)       # the index still answers
        assert np.array_equal(r1, r0) and np.array_equal(s1.view(np.int32), s0.view(np.int32))


# ---- store level: the native index behind MI355XVectorStore, a deterministic embeddings stub -----------------------------------------
class StubEmbeddings:
    """Unit vectors derived from the text's hash: no encoder, no fused query path."""
    dim = 384

    def _vec(self, text):
        seed = int.from_bytes(hashlib.sha256(text.encode()).digest()[:8], "little")
        v = np.random.default_rng(seed).standard_normal(self.dim)
        return (v / np.linalg.norm(v)).astype(np.float32)

    def embed_documents(self, texts):
        return [self._vec(t).tolist() for t in texts]

    def embed_query(self, text):
        # near a stored document, so the top of every list is well separated
        base = self._vec("doc %d" % (int(hashlib.md5(text.encode()).hexdigest(), 16) % 900))
        v = base + 0.3 * self._vec("noise " + text)
        return (v / np.linalg.norm(v)).astype(np.float32).tolist()


def _records(n=900):
    texts = ["doc %d" % i for i in range(n)]
    metas = [{"source": "%s.pdf" % "abc"[i % 3], "lang": ("en", "nl")[(i // 3) % 2], "page": i % 7} for i in range(n)]
    ids = ["pk%04d" % i for i in range(n)]
    return texts, metas, ids


def _store(rmu, keep=None):
    from ragmeup_amd.vectorstore import MI355XVectorStore
    texts, metas, ids = _records()
    sel = [i for i in range(len(texts)) if keep is None or keep(metas[i], ids[i])]
    st = MI355XVectorStore(embeddings=StubEmbeddings(), collection_name="subset-test", auto_persist=False)
    st.add_texts([texts[i] for i in sel], [metas[i] for i in sel], ids=[ids[i] for i in sel])
    return st


def _same_docs(a, b):
    assert [d.page_content for d in a] == [d.page_content for d in b]
    assert [d.metadata for d in a] == [d.metadata for d in b]
    assert len(a) > 0


FILTERS = [
    (dict(expr='source == "a.pdf"'), lambda m, pk: m["source"] == "a.pdf"),
    (dict(filter={"source": "b.pdf", "lang": "nl"}), lambda m, pk: m["source"] == "b.pdf" and m["lang"] == "nl"),
    (dict(expr="source in ['a.pdf', \"c.pdf\"] && lang == 'en'"), lambda m, pk: m["source"] in ("a.pdf", "c.pdf") and m["lang"] == "en"),
    (dict(filter={"page": [1, 2]}, expr='lang == "en"'), lambda m, pk: m["page"] in (1, 2) and m["lang"] == "en"),
    (dict(filter={"pk": ["pk0003", "pk0010", "pk0500"]}), lambda m, pk: pk in ("pk0003", "pk0010", "pk0500")),
]
QUERIES = ["what is a wave", "lane and tile", "hbm bandwidth", "top-10 answer", "naive cafe"]


@pytest.mark.parametrize("which", range(len(FILTERS)))
def test_store_filters_equal_a_store_of_the_matching_records(rmu, which):
    kw, keep = FILTERS[which]
    full, part = _store(rmu), _store(rmu, keep)
    for query in QUERIES:
        a = full.similarity_search_with_score(query, k=6, **kw)
        b = part.similarity_search_with_score(query, k=6)
        _same_docs([d for d, _ in a], [d for d, _ in b])
        assert all(keep(d.metadata, d.metadata["pk"]) for d, _ in a)
        assert np.abs(np.array([s for _, s in a]) - np.array([s for _, s in b])).max() <= 1e-4
        _same_docs(full.similarity_search(query, k=6, **kw), part.similarity_search(query, k=6))
        vec = StubEmbeddings().embed_query(query)
        _same_docs([d for d, _ in full.similarity_search_with_score_by_vector(vec, k=6, **kw)],
                   [d for d, _ in part.similarity_search_with_score_by_vector(vec, k=6)])
        ra = full.similarity_search_with_relevance_scores(query, k=6, **kw)
        rb = part.similarity_search_with_relevance_scores(query, k=6)
        _same_docs([d for d, _ in ra], [d for d, _ in rb])
        assert np.abs(np.array([s for _, s in ra]) - np.array([s for _, s in rb])).max() <= 1e-4
        for fetch_k in (20, 80):                         # device selection / the host selection above 64 candidates
            _same_docs(full.max_marginal_relevance_search(query, k=4, fetch_k=fetch_k, **kw),
                       part.max_marginal_relevance_search(query, k=4, fetch_k=fetch_k))
        _same_docs(full.max_marginal_relevance_search_by_vector(vec, k=4, fetch_k=20, **kw),
                   part.max_marginal_relevance_search_by_vector(vec, k=4, fetch_k=20))
        for st in ("similarity", "mmr"):
            _same_docs(full.as_retriever(search_type=st, search_kwargs={"k": 5, **kw}).invoke(query),
                       part.as_retriever(search_type=st, search_kwargs={"k": 5}).invoke(query))
    for a, b in zip(full.similarity_search_with_score_batch(QUERIES, k=6, **kw), part.similarity_search_with_score_batch(QUERIES, k=6)):
        _same_docs([d for d, _ in a], [d for d, _ in b])
        assert np.abs(np.array([s for _, s in a]) - np.array([s for _, s in b])).max() <= 1e-4
    for a, b in zip(full.max_marginal_relevance_search_batch(QUERIES, k=4, **kw), part.max_marginal_relevance_search_batch(QUERIES, k=4)):
        _same_docs(a, b)
    for st in ("similarity", "mmr"):
        for a, b in zip(full.as_retriever(search_type=st, search_kwargs={"k": 5, **kw}).batch_invoke(QUERIES),
                        part.as_retriever(search_type=st, search_kwargs={"k": 5}).batch_invoke(QUERIES)):
            _same_docs(a, b)


def test_store_filter_matching_nothing_and_bad_expressions(rmu):
    full = _store(rmu)
    assert full.similarity_search("a wave", k=4, expr='source == "nowhere.pdf"') == []
    assert full.max_marginal_relevance_search("a wave", k=4, filter={"lang": "fr"}) == []
    assert full.as_retriever(search_kwargs={"k": 3, "filter": {"source": "zzz"}}).invoke("a wave") == []
    for bad in ('source = "a.pdf"', "source == a.pdf and", 'page > 3', 'source == "a.pdf" or lang == "en"'):
        with pytest.raises(ValueError):
            full.similarity_search("a wave", k=4, expr=bad)


def test_store_filter_delete_compact_filter(rmu):
    keep = lambda m, pk: m["source"] == "a.pdf"
    full = _store(rmu)
    kw = dict(expr='source == "a.pdf"')
    first = full.similarity_search("lane and tile", k=6, **kw)
    assert len(first) == 6
    gone = [d.metadata["pk"] for d in first[:3]] + ["pk%04d" % i for i in range(0, 400, 2)]
    full.delete(ids=gone)
    part = _store(rmu, lambda m, pk: keep(m, pk) and pk not in set(gone))
    for query in QUERIES:
        _same_docs(full.similarity_search(query, k=6, **kw), part.similarity_search(query, k=6))
    assert full.compact() > 0
    for query in QUERIES:
        a = full.similarity_search_with_score(query, k=6, **kw)
        b = part.similarity_search_with_score(query, k=6)
        _same_docs([d for d, _ in a], [d for d, _ in b])
        assert np.abs(np.array([s for _, s in a]) - np.array([s for _, s in b])).max() <= 1e-4
        _same_docs(full.max_marginal_relevance_search(query, k=4, **kw), part.max_marginal_relevance_search(query, k=4))
