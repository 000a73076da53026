"""GPU: rmu_index_search_groups -- one row list per group of queries, every group in one call (scan_groups_kernel, the tile loop of the
gathered scan behind a per-workgroup work table) -- bit for bit against the per-list call it replaces, against the fp64 oracle run on
x[list], with device lists that name ids outside the index, across a compaction, and through the store's per-query filters.

ONE call holds every case: lists of 0, 1, 5 (shorter than k), 31, 32, 33, 127, 128, 129 and 1 037 rows and every row, two identical lists,
two overlapping ones, one nobody uses, one made of bit-identical rows; groups of 1, 2, 31, 32, 33 and 129 queries (both geometry classes).
Tolerance and tie rule of the oracle check are the project's own (tests/helpers.assert_topk_parity: ids identical, scores within 1e-4)."""
import numpy as np
import pytest

from oracle import oracle as O
from tests.helpers import assert_topk_parity

pytestmark = pytest.mark.gpu

N_ROWS = 4_099           # not a multiple of any tile
DUP_OF, N_DUP = 3, 20    # 20 rows are bit-identical copies of row 3
KS = (1, 10, 33, 112)
CASES = [(m, d) for m in ("ip", "cosine") for d in (64, 384, 768)] + [("l2", d) for d in (384, 700)]


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


def _layout():
    """-> (lists, q_list, dup rows, dead rows): the same for every case."""
    rng = np.random.default_rng(31)
    pick = lambda m: np.sort(rng.choice(N_ROWS, m, replace=False)).astype(np.int64)
    dup = np.sort(rng.choice(np.arange(10, N_ROWS), N_DUP, replace=False)).astype(np.int64)
    big = pick(1_037)
    lists = [pick(n) for n in (0, 1, 5, 31, 32, 33, 127, 128, 129)] + [big, np.arange(N_ROWS, dtype=np.int64)]
    lists.append(big.copy())                                                           # 11: identical to list 9
    lists.append(np.unique(np.concatenate([big[::2], pick(300)])).astype(np.int64))    # 12: overlaps list 9
    lists.append(pick(50))                                                             # 13: nobody uses it
    lists.append(np.unique(np.concatenate([dup, [DUP_OF], pick(200)])).astype(np.int64))   # 14: the copies, the tie rule decides
    groups = {0: 1, 1: 2, 2: 1, 3: 1, 4: 31, 5: 1, 6: 32, 7: 1, 8: 33, 9: 129, 10: 2, 11: 1, 12: 1, 14: 2}      # list -> queries
    q_list = np.concatenate([np.full(n, g) for g, n in groups.items()])
    q_list = q_list[np.random.default_rng(32).permutation(q_list.size)]               # any order: search_groups sorts
    keep = np.concatenate([dup, [DUP_OF], lists[1], lists[2]])
    dead = np.concatenate([rng.choice(big[~np.isin(big, keep)], 20, replace=False), rng.choice(np.setdiff1d(np.arange(N_ROWS), np.concatenate([keep, big])), 20, replace=False)])
    return lists, q_list, dup, np.unique(dead).astype(np.int64)


LISTS, Q_LIST, DUP, DEAD = _layout()
NQ = Q_LIST.size
FIRST_OF_14 = int(np.nonzero(Q_LIST == 14)[0][0])        # this query IS the copied row: its top N_DUP + 1 scores are equal


def _corpus(metric, dim):
    x = O.make_corpus(N_ROWS, dim, seed=2000 + dim)
    q, _ = O.make_queries(x, NQ, seed=91 + dim)
    if metric != "ip":
        x = (x * np.random.default_rng(6).uniform(0.5, 1.5, (N_ROWS, 1))).astype(np.float32)
    x[DUP] = x[DUP_OF]
    q = q.copy()
    q[FIRST_OF_14] = x[DUP_OF]
    return x, q


_CACHE = {}


def _case(rmu, metric, dim):
    """-> (index, x, q, {k: per-query results of idx.search(q_i, k, rows=list)}): built once per (metric, dim), one at a time in HBM."""
    key = (metric, dim)
    if key not in _CACHE:
        _CACHE.clear()
        x, q = _corpus(metric, dim)
        idx = rmu.FlatIndex(dim, metric=_metric(metric))
        idx.add(x[:1_500]); idx.add(x[1_500:])
        assert idx.remove_rows(DEAD) == DEAD.size == 40
        _CACHE[key] = (idx, x, q, {})
    return _CACHE[key]


def _per_list_reference(idx, q, k, lists=LISTS):
    s = np.empty((NQ, k), np.float32)
    r = np.empty((NQ, k), np.int64)
    for i in range(NQ):
        s[i], r[i] = (a[0] for a in idx.search(q[i:i + 1], k, rows=lists[Q_LIST[i]]))
    return s, r


def _reference(rmu, metric, dim, k):
    idx, x, q, refs = _case(rmu, metric, dim)
    if k not in refs:
        refs[k] = _per_list_reference(idx, q, k)
    return refs[k]


def _same(got, want, what):
    assert np.array_equal(got[1], want[1]), what
    assert np.array_equal(got[0].view(np.int32), want[0].view(np.int32)), what


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("metric,dim", CASES)
def test_one_call_equals_the_per_list_calls_bit_for_bit_and_the_fp64_oracle(rmu, metric, dim, k):
    idx, x, q, _ = _case(rmu, metric, dim)
    s, r = idx.search_groups(q, k, LISTS, Q_LIST)
    assert s.shape == (NQ, k) and r.shape == (NQ, k)
    # (e) at most two scan launches however many lists: one per geometry class present (k > 32: every group takes the 128-query class)
    passes = idx.last_geometry()["launches"]
    assert passes == (2 if k <= 32 else 1), passes
    # (a) the per-list calls
    _same((s, r), _reference(rmu, metric, dim, k), f"{metric} d={dim} k={k}")
    assert not np.isin(r[r >= 0], DEAD).any()
    # (b) the oracle on the live rows of each query's list
    m = _metric(metric)
    for g in np.unique(Q_LIST):
        rows = LISTS[g][~np.isin(LISTS[g], DEAD)]
        sel = np.nonzero(Q_LIST == g)[0]
        os_, op = O.flat_search(q[sel], x[rows], k + 8, metric=m)
        or_ = np.where(op >= 0, rows[np.maximum(op, 0)] if rows.size else -1, -1)
        try:
            assert_topk_parity(-s[sel] if metric == "l2" else s[sel], r[sel], os_, or_)
        except AssertionError as e:
            raise AssertionError(f"{metric} d={dim} k={k} list {g} ({LISTS[g].size} rows, {sel.size} queries): {e}") from None
        assert ((r[sel] >= 0).sum(1) == min(k, rows.size)).all(), (g, k)
    # the tie rule: equal scores come back lowest row first
    want = sorted([DUP_OF] + DUP.tolist())[:k]
    assert r[FIRST_OF_14, :len(want)].tolist() == want
    assert (s[FIRST_OF_14, :len(want)].view(np.int32) == s[FIRST_OF_14, :1].view(np.int32)).all()
    # row_base
    s2, r2 = idx.search_groups(q, k, LISTS, Q_LIST, row_base=1_000_000)
    _same((s2, r2), (s, np.where(r >= 0, r + 1_000_000, -1)), "row_base")


@pytest.mark.parametrize("metric,dim", [("ip", 384), ("l2", 700)])
def test_device_lists_with_ids_outside_the_index(rmu, metric, dim):
    import torch
    idx, x, q, _ = _case(rmu, metric, dim)
    rng = np.random.default_rng(41)
    wild = []
    for l in LISTS:
        junk = np.array([N_ROWS, N_ROWS + 5, 2 ** 31 + 7, 2 ** 40, -3], np.int64)
        at = np.sort(rng.integers(0, l.size + 1, junk.size))
        wild.append(torch.from_numpy(np.insert(l, at, junk)).cuda())
    for k in (10, 112):
        _same(idx.search_groups(q, k, wild, Q_LIST), _reference(rmu, metric, dim, k), f"device lists {metric} k={k}")
    with pytest.raises(ValueError):
        idx.search_groups(q, 10, [wild[0]] + LISTS[1:], Q_LIST)       # all host arrays or all device tensors


def test_the_same_call_after_compaction_returns_the_mapped_ids(rmu):
    x, q = _corpus("cosine", 384)
    idx = rmu.FlatIndex(384, metric=_metric("cosine"))
    idx.add(x[:1_500]); idx.add(x[1_500:])
    idx.remove_rows(DEAD)
    before = {k: idx.search_groups(q, k, LISTS, Q_LIST) for k in (10, 33)}
    m = idx.compact()
    assert len(idx) == N_ROWS - DEAD.size
    mapped = [m[l][m[l] >= 0] for l in LISTS]
    assert all((np.diff(l) > 0).all() for l in mapped)
    for k, (s, r) in before.items():
        _same(idx.search_groups(q, k, mapped, Q_LIST), (s, np.where(r >= 0, m[np.maximum(r, 0)], -1)), f"after compact k={k}")


def test_host_lists_and_arguments_are_checked_before_anything_runs(rmu):
    from ragmeup_amd import _native as N
    idx, x, q, _ = _case(rmu, "ip", 64)
    s0, r0 = idx.search_groups(q[:4], 5, LISTS, [9, 4, 9, 0])
    for bad in (LISTS[9][::-1].copy(), np.array([1, 2, 2, 3], np.int64), np.array([-1, 4, 9], np.int64), np.array([5, N_ROWS], np.int64)):
        with pytest.raises(N.RmuError) as e:
            idx.search_groups(q[:4], 5, [LISTS[9], bad], [0, 1, 0, 0])
        assert e.value.code == -1 and "list 1" in str(e.value)
    with pytest.raises(N.RmuError):
        idx.search_groups(q[:4], 113, LISTS, [9, 4, 9, 0])
    with pytest.raises(ValueError):
        idx.search_groups(q[:4], 5, LISTS, [9, 4, 9, len(LISTS)])
    _same(idx.search_groups(q[:4], 5, LISTS, [9, 4, 9, 0]), (s0, r0), "the index still answers")
    wide = rmu.FlatIndex(1024)
    with pytest.raises(ValueError):
        wide.search_groups(np.zeros((1, 1024), np.float32), 5, [np.arange(3)], [0])


# ---- (f) store level: per-query filters over hash embeddings ----------------------------------------------------------------------------
class HashEmbeddings:
    """Unit vectors derived from the text's hash, the same for a document and for a query: no encoder, no fused query path, and a batch
    (embed_documents) embeds a query exactly as the single call (embed_query) does."""
    dim = 384

    def _vec(self, text):
        import hashlib
        seed = int.from_bytes(hashlib.sha256(text.encode()).digest()[:8], "little")
        v = np.random.default_rng(seed).standard_normal(self.dim)
        return (v / np.linalg.norm(v)).astype(np.float32)

    def embed_documents(self, texts):
        return [self._vec(t).tolist() for t in texts]

    def embed_query(self, text):
        return self._vec(text).tolist()


def test_store_and_retriever_with_per_query_filters_equal_the_per_query_calls(rmu):
    from ragmeup_amd.vectorstore import MI355XVectorStore
    from tests.test_subset_gpu import QUERIES, _records
    texts, metas, ids = _records()
    st = MI355XVectorStore(embeddings=HashEmbeddings(), collection_name="groups-test", auto_persist=False)
    st.add_texts(texts, metas, ids=ids)
    assert hasattr(st._index, "search_groups")
    queries = QUERIES + ["a sixth one", "lane and tile"]
    exprs = ['source == "a.pdf"', None, 'source == "b.pdf" and lang == "nl"', 'source == "a.pdf"', 'source == "nowhere.pdf"', 'page == 3', None]
    filters = [{"source": "a.pdf"}, None, {"source": "b.pdf", "lang": "nl"}, {"source": "a.pdf"}, {"lang": "fr"}, {"page": 3}, None]
    docs = lambda ds: [(d.page_content, d.metadata) for d in ds]
    for name, one, conds in (("exprs", "expr", exprs), ("filters", "filter", filters)):
        kw = [{} if c is None else {one: c} for c in conds]
        want = [st.similarity_search_with_score(qy, k=6, **w) for qy, w in zip(queries, kw)]
        got = st.similarity_search_with_score_batch(queries, k=6, **{name: conds})
        assert [docs(d for d, _ in g) for g in got] == [docs(d for d, _ in w) for w in want]
        for g, w in zip(got, want):
            assert np.abs(np.array([s for _, s in g]) - np.array([s for _, s in w])).max(initial=0.0) <= 1e-4
        assert got[4] == [] and len(got[0]) == 6 and all(d.metadata["source"] == "a.pdf" for d, _ in got[0])
        assert [docs(g) for g in st.as_retriever(search_kwargs={"k": 6}).batch_invoke(queries, **{name: conds})] == [docs(d for d, _ in w) for w in want]
        for fetch_k in (20, 80):                         # the device selection / the host selection above 64 candidates
            want_mmr = [st.max_marginal_relevance_search(qy, k=4, fetch_k=fetch_k, **w) for qy, w in zip(queries, kw)]
            got_mmr = st.max_marginal_relevance_search_batch(queries, k=4, fetch_k=fetch_k, **{name: conds})
            assert [docs(g) for g in got_mmr] == [docs(w) for w in want_mmr]
        got_mmr = st.as_retriever(search_type="mmr", search_kwargs={"k": 4, "fetch_k": 20}).batch_invoke(queries, **{name: conds})
        assert [docs(g) for g in got_mmr] == [docs(w) for w in [st.max_marginal_relevance_search(qy, k=4, fetch_k=20, **w) for qy, w in zip(queries, kw)]]
    with pytest.raises(ValueError):
        st.similarity_search_with_score_batch(queries, k=6, expr=exprs[0], exprs=exprs)
