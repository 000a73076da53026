"""GPU: the device-side selection (rmu_columns_select: count, scan, write over code columns in HBM) against np.flatnonzero of the same
predicate, rmu_index_search_where against the per-query search(rows=host list) it replaces, and two stores over the same records -- one
with device_fields -- through every filtered entry point.  Every comparison is exact: np.array_equal on row ids and on the scores viewed
as uint32 (the lists are sets of integers and the scan is the existing one)."""

import numpy as np
import pytest

from oracle import oracle as O
from tests import where_cases as W

pytestmark = pytest.mark.gpu

SELS = W.selections()


@pytest.fixture(scope="module")
def rmu():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import ragmeup_amd
    from ragmeup_amd import _native
    _native.lib()
    return ragmeup_amd


_REF = {}


def _reference(n):
    """codes and the reference lists of every selection, computed once per row count"""
    if n not in _REF:
        codes = W.make_codes(n)
        _REF[n] = (codes, [W.reference(codes, s) for s in SELS])
    return _REF[n]


@pytest.mark.parametrize("tile", (0, 64))
@pytest.mark.parametrize("n", W.ROW_COUNTS)
def test_select_equals_flatnonzero(rmu, n, tile):
    from ragmeup_amd import _native as N
    from ragmeup_amd.index import flatten_selections
    codes, want = _reference(n)
    c = rmu.Columns(W.N_FIELDS)
    c.append(codes[:n // 2]); c.append(codes[n // 2:])
    c.set_tile_rows(tile)
    assert len(SELS) == 33
    ptr = np.concatenate([[0], np.cumsum([w.size for w in want])]).astype(np.int64)
    # HOST output, all 33 selections in one call
    got = c.select(SELS)
    for g in range(len(SELS)):
        assert got[g].dtype == np.int64 and np.array_equal(got[g], want[g]), (n, tile, g)
    assert want[6].size == 0 and want[12].size == 0 and want[7].size == n and np.array_equal(want[10], want[4])
    assert want[9].tolist() == [n - 1] and want[8].tolist() == ([0] if n > 1 else [])
    # count only
    assert np.array_equal(c.select(SELS, count_only=True), ptr)
    # DEVICE output
    dev = c.select(SELS, device=True)
    for g in range(len(SELS)):
        assert np.array_equal(dev[g].cpu().numpy(), want[g]), (n, tile, g)
    # one selection at a time (1, 2 and 4 terms), and a call whose lists are all empty
    for g in (0, 4, 5):
        assert np.array_equal(c.select([SELS[g]])[0], want[g])
    assert [x.size for x in c.select([SELS[6], SELS[12]])] == [0, 0]
    # out_cap one short: -1, list_ptr still correct, nothing written
    terms, cs, sp = flatten_selections(SELS)
    lp = np.full(len(SELS) + 1, -7, np.int64)
    out = np.full(int(ptr[-1]), -7, np.int64)
    lib = N.lib()
    rc = lib.rmu_columns_select(c._h, terms.ctypes.data, terms.shape[0], cs.ctypes.data, sp.ctypes.data, len(SELS), 0, out.ctypes.data,
                                int(ptr[-1]) - 1, lp.ctypes.data, 0)
    assert rc == -1 and b"out_cap" in lib.rmu_last_error()
    assert np.array_equal(lp, ptr) and (out == -7).all()
    rc = lib.rmu_columns_select(c._h, terms.ctypes.data, terms.shape[0], cs.ctypes.data, sp.ctypes.data, len(SELS), 0, out.ctypes.data,
                                int(ptr[-1]), lp.ctypes.data, 0)
    assert rc == 0 and np.array_equal(out, np.concatenate(want))
    c.close()


def test_select_follows_append_and_compact(rmu):
    """the tail upload, a re-allocation of the image, and a compaction, at both tile sizes"""
    codes, _ = _reference(4097)
    c = rmu.Columns(W.N_FIELDS)
    assert [x.size for x in c.select(SELS[:3])] == [0, 0, 0]                   # no rows: no launch
    c.append(codes[:1000])
    check = lambda have: all(np.array_equal(g, W.reference(have, s)) for g, s in zip(c.select(SELS), SELS))
    assert check(codes[:1000])
    c.append(codes[1000:1100])                                                 # fits the image: only the tail is uploaded
    assert check(codes[:1100])
    c.append(codes[1100:])                                                     # 4 097 rows: the image is re-allocated
    assert check(codes)
    dead = np.unique(np.random.default_rng(3).integers(0, 4097, 500))
    m, after = W.compact_reference(codes, dead)
    assert c.compact(m) == after.shape[0]
    for tile in (64, 0):
        c.set_tile_rows(tile)
        assert check(after)
    c.close()


# ---- rmu_index_search_where against search(rows=host list) per query --------------------------------------------------------------------
N_ROWS = 4_100
EXTRA = 4_000              # rows appended later: see the re-allocation below
# (selection, queries): groups of 1, 33 and 129 queries -- both geometry classes of the gathered scan, as in tests/test_groups_gpu.py --,
# an empty selection, one that holds row 0 alone (fewer rows than k), one that holds every row
GROUPS = ((0, 1), (4, 33), (3, 129), (6, 1), (8, 1), (7, 2), (11, 33), (12, 1))
Q_SEL = np.concatenate([np.full(cnt, g) for g, cnt in GROUPS])
Q_SEL = Q_SEL[np.random.default_rng(8).permutation(Q_SEL.size)]               # any order: search_where sorts
NQ = Q_SEL.size


def _same(got, want, what):
    assert np.array_equal(got[1], want[1]), what
    assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)), what


def _per_query(idx, q, k, codes):
    lists = {g: W.reference(codes, SELS[g]) for g, _ in GROUPS}
    s = np.empty((NQ, k), np.float32)
    r = np.empty((NQ, k), np.int64)
    for i in range(NQ):
        s[i], r[i] = (a[0] for a in idx.search(q[i:i + 1], k, rows=lists[int(Q_SEL[i])]))
    return s, r


@pytest.mark.parametrize("metric,dim", [("ip", 64), ("ip", 384), ("l2", 64), ("l2", 384)])
def test_search_where_equals_the_per_query_subset_search(rmu, metric, dim):
    from ragmeup_amd import _native as N
    m = {"ip": N.METRIC_IP, "l2": N.METRIC_L2SQ}[metric]
    x = O.make_corpus(N_ROWS + EXTRA, dim, seed=700 + dim)
    if metric == "l2":
        x = (x * np.random.default_rng(6).uniform(0.5, 1.5, (x.shape[0], 1))).astype(np.float32)
    q, _ = O.make_queries(x, NQ, seed=17 + dim)
    codes = W.make_codes(N_ROWS + EXTRA)
    idx = rmu.FlatIndex(dim, metric=m)
    cols = rmu.Columns(W.N_FIELDS)
    idx.add(x[:N_ROWS]); cols.append(codes[:N_ROWS])
    have = codes[:N_ROWS]

    def check(what, tile=0):
        cols.set_tile_rows(tile)
        for k in (5, 40):
            got = idx.search_where(q, k, cols, SELS, Q_SEL)
            assert got[0].shape == (NQ, k) and got[1].shape == (NQ, k)
            _same(got, _per_query(idx, q, k, have), f"{what} {metric} d={dim} k={k} tile={tile}")
        return got
    check("fresh")
    # tombstoned rows inside the selections: they keep their codes and never appear
    rng = np.random.default_rng(9)
    dead = np.unique(np.concatenate([rng.choice(W.reference(have, SELS[4]), 25, replace=False), rng.integers(1, N_ROWS, 200)]))
    assert idx.remove_rows(dead) == dead.size
    s, r = check("tombstones", tile=64)
    assert not np.isin(r[r >= 0], dead).any()
    # the padding: an empty selection, a term without codes, and row 0 alone with k = 40
    worst = np.inf if metric == "l2" else -np.inf
    for g in (6, 12):
        i = int(np.nonzero(Q_SEL == g)[0][0])
        assert (r[i] == -1).all() and (s[i] == worst).all()
    i = int(np.nonzero(Q_SEL == 8)[0][0])
    assert r[i].tolist() == [0] + [-1] * 39 and (s[i, 1:] == worst).all()
    # row_base
    s2, r2 = idx.search_where(q, 40, cols, SELS, Q_SEL, row_base=1_000_000)
    _same((s2, r2), (s, np.where(r >= 0, r + 1_000_000, -1)), "row_base")
    # compact both
    mp = idx.compact()
    assert cols.compact(mp) == len(idx) == N_ROWS - dead.size
    have = have[mp >= 0]
    check("compacted")
    # append to both: a tail upload, then a re-allocation of the image INSIDE search_where.  The first upload (4 100 rows) allocated
    # n + n / 4 + 1024 rounded up to a multiple of 1024 = 7 168 rows per field and the compaction kept that allocation (at least 3 875 rows
    # are left: at most 225 were dead); 50 more rows fit it, EXTRA - 50 = 3 950 more make at least 7 875: the image no longer fits
    first_cap = (N_ROWS + N_ROWS // 4 + 1024 + 1023) // 1024 * 1024
    lo = N_ROWS
    for cnt in (50, EXTRA - 50):
        idx.add(x[lo:lo + cnt]); cols.append(codes[lo:lo + cnt])
        have = np.concatenate([have, codes[lo:lo + cnt]])
        lo += cnt
        assert (len(cols) <= first_cap) == (cnt == 50)
        check(f"appended {cnt}", tile=64 if cnt == 50 else 0)
    # columns one row short of the index: refused, and the index still answers
    short = rmu.Columns(W.N_FIELDS)
    short.append(have[:-1])
    with pytest.raises(N.RmuError) as e:
        idx.search_where(q, 5, short, SELS, Q_SEL)
    assert e.value.code == -1 and "out of step" in str(e.value)
    want = idx.search_where(q, 5, cols, SELS, Q_SEL)
    _same(want, _per_query(idx, q, 5, have), "after the refusal")
    # every query on selections without rows: no scan, all padding
    s0, r0 = idx.search_where(q[:3], 5, cols, [SELS[6], SELS[12]], [1, 0, 1])
    assert (r0 == -1).all() and (s0 == worst).all()
    short.close(); cols.close(); idx.close()


def test_search_where_refuses_a_wide_index_and_sends_blocks(rmu):
    from ragmeup_amd import _native as N
    from ragmeup_amd.index import flatten_selections
    wide = rmu.FlatIndex(1024)
    wide.add(np.ones((4, 1024), np.float32))
    cols = rmu.Columns(1)
    cols.append(np.zeros((4, 1), np.int32))
    with pytest.raises(ValueError):
        wide.search_where(np.zeros((1, 1024), np.float32), 2, cols, [[(0, [0])]], [0])
    terms, cs, sp = flatten_selections([[(0, [0])]])
    q = np.zeros((1, 1024), np.float32)
    s, r, qs = np.zeros((1, 2), np.float32), np.zeros((1, 2), np.int64), np.zeros(1, np.int32)
    lib = N.lib()
    rc = lib.rmu_index_search_where(wide._h, cols._h, q.ctypes.data, 1, 2, 0, 0, terms.ctypes.data, 1, cs.ctypes.data, sp.ctypes.data, 1,
                                    qs.ctypes.data, s.ctypes.data, r.ctypes.data, 0)
    assert rc == -1 and b"768" in lib.rmu_last_error()
    # more queries than one call takes: two blocks, each with the selections it names
    idx = rmu.FlatIndex(64)
    x = O.make_corpus(300, 64, seed=4)
    idx.add(x)
    c2 = rmu.Columns(W.N_FIELDS)
    codes = W.make_codes(300)
    c2.append(codes)
    nq = N.MAX_QUERIES_PER_CALL + 5
    qq = np.tile(x[:7], (nq // 7 + 1, 1))[:nq]
    q_sel = (np.arange(nq) * 5) % 4
    s, r = idx.search_where(qq, 3, c2, [SELS[0], SELS[1], SELS[7], SELS[6]], q_sel)
    for g, sel in enumerate((SELS[0], SELS[1], SELS[7])):
        rows = W.reference(codes, sel)
        pick = np.nonzero(q_sel == g)[0][:7]
        ws, wr = idx.search(qq[pick], 3, rows=rows)
        _same((s[pick], r[pick]), (ws, wr), f"block selection {g}")
    assert (r[q_sel == 3] == -1).all()
    # 9 000 selections of which two are named: only those reach the library (it takes at most 8 192 per call)
    many = [[(0, [g % 7]), (1, [g % 300])] for g in range(9_000)]
    many[0], many[8_999] = SELS[1], SELS[7]
    s, r = idx.search_where(qq[:7], 3, c2, many, [8_999, 0, 0, 8_999, 0, 8_999, 0])
    for g, sel in ((0, SELS[1]), (8_999, SELS[7])):
        pick = [i for i, v in enumerate([8_999, 0, 0, 8_999, 0, 8_999, 0]) if v == g]
        _same((s[pick], r[pick]), idx.search(qq[pick], 3, rows=W.reference(codes, sel)), f"selection {g} of 9 000")


# ---- two stores over the same records -------------------------------------------------------------------------------------------------
def _docs(ds):
    return [(d.page_content, d.metadata) for d in ds]


def _compare(host, dev):
    a = host.similarity_search_with_score_batch(W.QUERIES, k=6, exprs=W.EXPRS)
    b = dev.similarity_search_with_score_batch(W.QUERIES, k=6, exprs=W.EXPRS)
    assert [_docs(d for d, _ in g) for g in b] == [_docs(d for d, _ in g) for g in a]
    assert [[s for _, s in g] for g in b] == [[s for _, s in g] for g in a]              # equal scores, not close ones
    assert b[3] == [] and len(b[0]) == 6 and all(d.metadata["source"] == "a.pdf" for d, _ in b[0])
    for fetch_k in (20, 80):
        assert ([_docs(g) for g in dev.max_marginal_relevance_search_batch(W.QUERIES, k=4, fetch_k=fetch_k, exprs=W.EXPRS)] ==
                [_docs(g) for g in host.max_marginal_relevance_search_batch(W.QUERIES, k=4, fetch_k=fetch_k, exprs=W.EXPRS)])
    one = dev.similarity_search(W.QUERIES[0], k=8, expr=W.ONE_EXPR)
    assert _docs(one) == _docs(host.similarity_search(W.QUERIES[0], k=8, expr=W.ONE_EXPR)) and len(one) == 8
    flt = {"lang": ["nl", "de"], "source": "e.pdf"}
    scored = lambda st: [(d.page_content, d.metadata, s) for d, s in st.similarity_search_with_score(W.QUERIES[1], k=5, filter=flt)]
    assert scored(dev) == scored(host) and len(scored(dev)) == 5
    assert _docs(dev.max_marginal_relevance_search(W.QUERIES[2], k=3, expr='lang == "de"')) == _docs(host.max_marginal_relevance_search(W.QUERIES[2], k=3, expr='lang == "de"'))


def test_a_store_with_device_fields_answers_like_the_store_without(rmu, tmp_path):
    from ragmeup_amd.vectorstore import MI355XVectorStore
    texts, metas, ids = W.records()
    mk = lambda name, **kw: MI355XVectorStore(embeddings=W.HashEmbeddings(), collection_name=name, auto_persist=False,
                                               connection=str(tmp_path / "where.db"), **kw)
    host, dev = mk("host"), mk("dev", device_fields=("source", "lang"))
    for st in (host, dev):
        st.add_texts(texts, metas, ids=ids)
    assert hasattr(dev._index, "search_where") and len(dev._columns) == len(dev._index) == 3000 and host._columns is None
    _compare(host, dev)
    assert dev._field_map_builds == 0 and host._field_map_builds > 0
    for st in (host, dev):                                   # upsert
        st.add_texts(texts[100:160], [dict(m, source="a.pdf", lang="nl") for m in metas[100:160]], ids=ids[100:160])
    assert len(dev._columns) == len(dev._index) == 3060
    _compare(host, dev)
    assert dev._field_map_builds == 0
    for st in (host, dev):
        assert st.delete(expr='source == "c.pdf"').delete_count > 0
    assert dev._field_map_builds == 1                        # delete(expr=) keeps the host maps
    _compare(host, dev)
    for st in (host, dev):
        assert st.compact() > 0
    assert len(dev._columns) == len(dev._index) == len(host._index)
    _compare(host, dev)
    for st in (host, dev):
        assert st.persist()
    host2, dev2 = mk("host"), mk("dev", device_fields=("source", "lang"))
    assert host2.load() and dev2.load() and len(dev2._columns) == len(dev2._index)
    _compare(host2, dev2)
    _compare(host, dev2)
    assert dev._field_map_builds == 1 and dev2._field_map_builds == 0
