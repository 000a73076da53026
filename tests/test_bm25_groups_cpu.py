"""CPU: rmu_bm25_search_groups (include/rmu.h) -- the symbol, every refusal that needs no device, the answers that need none, the host
plan (rmu_bm25_groups_plan_) over the list families of tests/bm25_groups.py, and the Python surface over stand-ins: BM25Index.search_groups'
ordering, the retriever's per-request conditions and field-map cache, and the plurals of the ensemble and the hybrid retriever."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests.bm25_groups import SIZES, TILE, assignment, case_lists, plan, removed_of

NAME = "rmu_bm25_search_groups"


def _ptr(a):
    return a.ctypes.data


def test_the_symbol_is_declared_exported_and_bound(librmu):
    from ragmeup_amd import _native
    header = open(os.path.join(os.path.dirname(_native.__file__), "..", "include", "rmu.h"), encoding="utf-8").read()
    assert re.search(r"\bint\s+%s\s*\(" % NAME, header)
    assert NAME in _native.SYMBOLS and hasattr(librmu, NAME)
    assert librmu.rmu_bm25_search_groups.argtypes is not None and len(librmu.rmu_bm25_search_groups.argtypes) == 13
    assert "rmu_bm25_groups_plan_" not in header and hasattr(librmu, "rmu_bm25_groups_plan_")


def _host_index(librmu, texts=(b"a b\0b c\0c\0", 10, 3)):
    h = ctypes.c_void_p()
    assert librmu.rmu_bm25_create(ctypes.byref(h), 1.5, 0.75, 0.25) == 0
    assert librmu.rmu_bm25_add_texts(h, texts[0], texts[1], texts[2], None) == 0
    return h


def test_refusals_that_need_no_device(librmu):
    h = _host_index(librmu)
    s, r = np.zeros(8, np.float32), np.zeros(8, np.int64)
    docs, ptr, ql = np.array([0, 2, 1], np.int64), np.array([0, 2, 3], np.int64), np.array([0, 1], np.int32)

    def call(h=h, blob=b"a\0b\0", bytes_=4, nq=2, k=4, docs=_ptr(docs), ptr=_ptr(ptr), n_lists=2, ql=_ptr(ql), s=_ptr(s), r=_ptr(r)):
        return librmu.rmu_bm25_search_groups(h, blob, bytes_, nq, k, 0, docs, ptr, n_lists, ql, s, r, 0)

    try:
        for kw in ({"h": None}, {"blob": None}, {"docs": None}, {"ptr": None}, {"ql": None}, {"s": None}, {"r": None}):
            assert call(**kw) == -1, kw
            assert b"null argument" in librmu.rmu_last_error(), kw
        assert call(nq=0) == -1 and call(nq=65536) == -1 and b"nq" in librmu.rmu_last_error()
        assert call(k=0) == -1 and call(k=113) == -1 and b"RMU_MAX_K" in librmu.rmu_last_error()
        assert call(blob=b"a\0b", bytes_=3) == -1
        assert call(n_lists=0) == -1 and b"n_lists" in librmu.rmu_last_error()
        for bad_ptr, what in (([1, 2, 3], b"list_ptr[0]"), ([0, 2, 1], b"non-decreasing")):
            p = np.array(bad_ptr, np.int64)
            assert call(ptr=_ptr(p)) == -1 and what in librmu.rmu_last_error(), bad_ptr
        for bad_ql in ([1, 0], [0, 2], [-1, 0]):
            q = np.array(bad_ql, np.int32)
            assert call(ql=_ptr(q)) == -1 and b"q_list" in librmu.rmu_last_error(), bad_ql
        # the lists, against an index that has never seen the device: not ascending inside a list, outside [0, DOCS)
        for bad_docs in ([2, 0, 1], [0, 0, 1], [0, 3, 1], [-1, 2, 1], [0, 2, 3]):
            d = np.array(bad_docs, np.int64)
            assert call(docs=_ptr(d)) == -1 and b"ascending" in librmu.rmu_last_error(), bad_docs
        # an unused list is checked all the same
        q0 = np.array([0, 0], np.int32)
        d = np.array([0, 2, 5], np.int64)
        assert call(docs=_ptr(d), ql=_ptr(q0)) == -1
        # lists may descend from one to the next: [0, 2] and [1] are fine -- and with nothing to launch they answer on the host
        e = np.array([0, 0, 0], np.int64)
        assert call(ptr=_ptr(e)) == 0 and np.all(np.isneginf(s)) and np.all(r == -1)
    finally:
        assert librmu.rmu_bm25_free(h) == 0


def test_nothing_live_and_empty_lists_answer_without_the_device(librmu):
    from ragmeup_amd.bm25 import BM25Index
    ix = BM25Index()
    try:
        ix.add_texts(["a b", "b c", "c", "d"])
        # every used list empty (the unused one is not): padding only
        s, d = ix.search_groups(["a", "c b", ""], 3, [np.array([], np.int64), np.arange(4), np.array([], np.int64)], [0, 2, 0])
        assert s.shape == (3, 3) and s.dtype == np.float32 and d.dtype == np.int64
        assert np.all(np.isneginf(s)) and np.all(d == -1)
        # used lists that hold removed documents only
        assert ix.remove([1, 3]) == 2
        s, d = ix.search_groups(["a", "c"], 2, [np.array([1, 3]), np.array([3])], [1, 0])
        assert np.all(np.isneginf(s)) and np.all(d == -1)
        # nothing live at all
        assert ix.remove([0, 2]) == 2
        s, d = ix.search_groups(["a", "c"], 5, [np.arange(4), np.array([2])], [0, 1])
        assert np.all(np.isneginf(s)) and np.all(d == -1)
        with pytest.raises(ValueError):
            ix.search_groups(["a"], 2, [np.arange(4)], [1])
        with pytest.raises(ValueError):
            ix.search_groups(["a", "b"], 2, [np.arange(4)], [0])
    finally:
        ix.close()


# ---- the plan ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("cap", [1, 3, 1024])
def test_the_plan_covers_every_live_candidate_once_within_the_part_cap(librmu, n, cap):
    removed = removed_of(n)
    live = np.ones(n, np.uint8)
    live[removed] = 0
    cases = case_lists(n, removed)
    names = list(cases)
    lists = [cases[name] for name in names]
    ql = np.sort(assignment(names, 40, seed=n))
    rc, work, mask, counts = plan(librmu, n, live, TILE, cap, lists, ql)
    assert rc == 0
    assert counts[0] == work.shape[0] and counts[1] == mask.size
    by_query = {i: work[work[:, 0] == i] for i in range(ql.size)}
    assert sum(w.shape[0] for w in by_query.values()) == work.shape[0]
    assert counts[3] == max(w.shape[0] for w in by_query.values())
    mask_of_list: dict = {}
    for i, w in by_query.items():
        ids = lists[ql[i]]
        cand = ids[live[ids] == 1]
        assert w.shape[0] <= cap and np.array_equal(w[:, 1], np.arange(w.shape[0])), (i, w)          # parts are numbered from 0, within the cap
        lo, hi = w[:, 2].astype(np.int64), w[:, 3].astype(np.int64)
        assert np.all(lo % TILE == 0) and np.all(lo < hi) and np.all(hi <= n) and np.all((hi % TILE == 0) | (hi == n))
        assert np.all(lo[1:] >= hi[:-1])                                                            # ascending, no overlap
        inside = ((cand[:, None] >= lo[None, :]) & (cand[:, None] < hi[None, :])).sum(axis=1)
        assert np.all(inside == 1), (names[ql[i]], cand[inside != 1])
        if cand.size == 0:
            assert w.shape[0] == 0                                                                  # no live candidate: no workgroup
        if cap == 1024:                                                                             # no tile without a candidate
            tiles = np.concatenate([np.arange(a // TILE, -(-b // TILE)) for a, b in zip(lo, hi)]) if w.shape[0] else np.zeros(0, np.int64)
            assert np.array_equal(tiles, np.unique(cand // TILE)), names[ql[i]]
        # the mask words of the ranges are allow AND live, zero elsewhere (joined empty tiles, the words past the end)
        for (_, _, a, b, off) in w.tolist():
            words = 2 * -(-(b - a) // 64)
            assert off + words <= mask.size
            bits = np.unpackbits(mask[off:off + words].view(np.uint8), bitorder="little")
            want = np.zeros(words * 32, np.uint8)
            want[cand[(cand >= a) & (cand < b)] - a] = 1
            assert np.array_equal(bits, want), (names[ql[i]], a, b)
        # the queries of one list share its mask words (and its ranges)
        key = tuple(map(tuple, w[:, 2:].tolist()))
        assert mask_of_list.setdefault(int(ql[i]), key) == key
    # only kept ranges have mask words: never n_lists x N / 32
    used = sorted(set(ql.tolist()))
    assert mask.size == sum(2 * -(-(b - a) // 64) for g in used for (a, b, _) in mask_of_list[g])
    if cap == 1024:
        assert counts[2] == sum(np.unique(lists[g][live[lists[g]] == 1] // TILE).size for g in used)


def test_a_long_list_spreads_over_parts_and_a_small_cap_joins_across_empty_tiles(librmu):
    n = 64 * 40
    live = np.ones(n, np.uint8)
    whole = np.arange(n)
    rc, work, _, counts = plan(librmu, n, live, TILE, 8, [whole], [0])
    assert rc == 0 and work.shape[0] == 8 and np.all(work[:, 3] - work[:, 2] == 5 * TILE)              # 40 kept tiles, 5 per part
    islands = np.concatenate([np.arange(t * TILE, t * TILE + 3) for t in (0, 9, 20, 21, 39)])
    rc, work, mask, counts = plan(librmu, n, live, TILE, 2, [islands], [0])
    assert rc == 0 and counts[2] == 5
    assert work[:, 2:4].tolist() == [[0, 10 * TILE], [20 * TILE, 40 * TILE]]                            # 4 pieces, joined two by two
    assert int(np.unpackbits(mask.view(np.uint8)).sum()) == islands.size


def test_the_planner_refuses_what_the_call_refuses(librmu):
    live = np.ones(10, np.uint8)
    assert plan(librmu, 10, live, TILE, 4, [np.array([3, 2])], [0])[0] == -1
    assert plan(librmu, 10, live, TILE, 4, [np.array([10])], [0])[0] == -1
    assert plan(librmu, 10, live, TILE, 4, [np.array([1])], [1])[0] == -1
    assert plan(librmu, 10, live, 48, 4, [np.array([1])], [0])[0] == -1
    assert plan(librmu, 10, live, TILE, 0, [np.array([1])], [0])[0] == -1
    assert plan(librmu, 10, live, TILE, 1025, [np.array([1])], [0])[0] == -1


# ---- BM25Index.search_groups: the caller's order, only the used lists ----------------------------------------------------------------------
def test_search_groups_restores_the_order_and_sends_only_the_used_lists(librmu, monkeypatch):
    from ragmeup_amd.bm25 import BM25Index
    ix = BM25Index()
    calls = []

    def fake(queries, k, docs, list_ptr, q_list, doc_base, stream):
        calls.append((list(queries), docs.copy(), list_ptr.copy(), q_list.copy(), doc_base, stream))
        assert q_list.dtype == np.int32 and list_ptr.dtype == np.int64 and docs.dtype == np.int64
        s = np.zeros((len(queries), k), np.float32)
        d = np.zeros((len(queries), k), np.int64)
        for i, q in enumerate(queries):                       # the answer names the query and the first id of its list
            s[i], d[i] = float(q[1:]), docs[list_ptr[q_list[i]]]
        return s, d

    monkeypatch.setattr(ix, "_groups_call", fake)
    try:
        lists = [np.array([100, 101]), np.array([200]), np.array([300, 301, 302]), np.array([400]), np.array([500])]
        ql = [3, 1, 3, 2, 1, 2]                                # lists 0 and 4 go unused; 0 lies outside the used range, 4 too
        s, d = ix.search_groups([f"q{i}" for i in range(6)], 2, lists, ql, doc_base=7, stream=5)
        assert len(calls) == 1
        queries, docs, ptr, q_list, base, stream = calls[0]
        assert queries == ["q1", "q4", "q3", "q5", "q0", "q2"]                  # sorted by list, stable
        assert docs.tolist() == [200, 300, 301, 302, 400] and ptr.tolist() == [0, 1, 4, 5] and q_list.tolist() == [0, 0, 1, 1, 2, 2]
        assert base == 7 and stream == 5
        assert s[:, 0].tolist() == [0, 1, 2, 3, 4, 5] and d[:, 0].tolist() == [400, 200, 400, 300, 200, 300]
        s, d = ix.search_groups([], 3, lists, [])
        assert s.shape == (0, 3) and d.shape == (0, 3) and len(calls) == 1
    finally:
        ix.close()


# ---- the retriever over a stand-in index -----------------------------------------------------------------------------------------------
class _Index:
    """records its calls; an answer is the query's length-th .. candidates of the list in turn, so it depends on query and list only"""

    def __init__(self, n=0):
        self.n, self.calls = n, []

    def add_texts(self, texts):
        first, self.n = self.n, self.n + len(list(texts))
        return first

    def remove(self, ids):
        return len(ids)

    def compact(self):
        raise AssertionError("not used")

    @staticmethod
    def _row(q, k, ids):
        ids = np.asarray(ids, np.int64)
        out = np.full(k, -1, np.int64)
        take = np.roll(ids, -(len(q) % max(ids.size, 1)))[:k]
        out[:take.size] = take
        return out

    def search(self, queries, k, docs=None, **kw):
        self.calls.append(("search" if docs is None else "subset", len(queries)))
        ids = np.arange(self.n) if docs is None else docs
        rows = np.stack([self._row(q, k, ids) for q in queries])
        return np.zeros(rows.shape, np.float32), rows

    def search_groups(self, queries, k, lists, q_list, **kw):
        self.calls.append(("groups", len(queries), len(lists)))
        rows = np.stack([self._row(q, k, lists[g]) for q, g in zip(queries, q_list)])
        return np.zeros(rows.shape, np.float32), rows


def _retriever(**kw):
    from ragmeup_amd.bm25 import MI355XBM25Retriever
    texts = [f"doc{i} common word{i % 3}" for i in range(12)]
    metas = [{"row": i, "source": f"f{i % 4}.pdf", "page": i % 2} for i in range(12)]
    r = MI355XBM25Retriever(vectorizer=_Index(), docs=[], k=3, **kw)
    r.add_texts(texts, metas, ids=[f"id-{i}" for i in range(12)])
    return r


def test_retriever_per_query_conditions_equal_the_per_query_calls():
    qs = ["a", "bb", "ccc", "dddd", "eeeee", "ffffff"]
    exprs = ['source == "f1.pdf"', None, 'source == "f2.pdf"', 'source == "f1.pdf"', 'source == "nowhere.pdf"', 'page == 1 and source == "f3.pdf"']
    r = _retriever()
    got = r.batch_invoke(qs, exprs=exprs)
    calls = r.vectorizer.calls
    assert calls == [("search", 1), ("groups", 4, 3)]                       # one unfiltered query, three distinct non-empty lists, one call
    for q, e, row in zip(qs, exprs, got):
        one = _retriever(search_kwargs={} if e is None else {"expr": e})
        assert [d.page_content for d in row] == [d.page_content for d in one.batch_invoke([q])[0]], (q, e)
        if e and "f1" in e:
            assert row and all(d.metadata["source"] == "f1.pdf" for d in row)
    assert got[4] == []
    # filters= say the same; both together are intersected per query
    flt = [{"source": "f1.pdf"}, None, {"source": "f2.pdf"}, {"source": "f1.pdf"}, {"source": "nowhere.pdf"}, {"page": 1, "source": "f3.pdf"}]
    assert [[d.page_content for d in row] for row in r.batch_invoke(qs, filters=flt)] == [[d.page_content for d in row] for row in got]
    both = r.batch_invoke(qs[:2], exprs=['source == "f1.pdf"', None], filters=[{"row": [1, 5]}, {"row": [2]}])
    assert [d.metadata["row"] for d in both[0]] == [5, 1] and [d.metadata["row"] for d in both[1]] == [2]


def test_retriever_routes():
    r = _retriever()
    calls = r.vectorizer.calls
    r.batch_invoke(["a", "b"], exprs=[None, None])
    assert calls == [("search", 2)]                                          # all None: one ordinary search
    del calls[:]
    r.batch_invoke(["a", "b", "c"], exprs=['source == "f1.pdf"'] * 2 + [None])
    assert calls == [("search", 1), ("subset", 2)]                           # one distinct list: the subset call
    del calls[:]
    r.batch_invoke(["a", "b"], filters=[{"source": "nowhere.pdf"}, {"source": "f0.pdf"}])
    assert calls == [("subset", 1)]                                          # an empty selection costs no launch
    del calls[:]
    r.batch_invoke(["a", "b", "c"], filters=[{"source": "f0.pdf"}, {"source": "f1.pdf"}, {"source": "f0.pdf"}])
    assert calls == [("groups", 3, 2)]                                       # two distinct lists: one grouped call
    del calls[:]
    assert r.batch_invoke([], exprs=[]) == [] and calls == []
    for bad in ({"exprs": ["a == 1"]}, {"filters": [None] * 3}, {"exprs": 'source == "f1.pdf"'}):
        with pytest.raises(ValueError):
            r.batch_invoke(["a", "b"], **bad)
    with pytest.raises(ValueError):
        r.batch_invoke(["a"], exprs=["row > 3"])
    # a singular form in search_kwargs and a plural form together
    for skw in ({"expr": 'source == "f1.pdf"'}, {"filter": {"page": 0}}):
        one = _retriever(search_kwargs=skw)
        with pytest.raises(ValueError):
            one.batch_invoke(["a"], exprs=[None])
        with pytest.raises(ValueError):
            one.batch_invoke(["a"], filters=[{"page": 1}])


def test_the_rule_is_the_measured_one():
    """profiles/bm25_groups.md is where GROUPS_RULE comes from: the grouped call where the table has it ahead in every run, else the loop"""
    from ragmeup_amd.bm25 import MI355XBM25Retriever as R
    assert R.GROUPS_RULE == ((1_000, 2, 128), (10_000, 8, 128), (100_000, 8, 32))
    use = lambda n_lists, docs, index=None: R._use_groups(index or _Index(), [np.arange(docs)] * n_lists)
    assert not use(1, 10) and use(2, 10) and use(128, 1_000) and not use(129, 1_000)
    assert not use(2, 1_001) and not use(7, 10_000) and use(8, 1_001) and use(128, 10_000)
    assert not use(7, 100_000) and use(8, 10_001) and use(32, 100_000) and not use(33, 100_000) and not use(8, 100_001)
    assert R._use_groups(_Index(), [np.arange(3), np.arange(1_000)]) and not R._use_groups(_Index(), [np.arange(3), np.arange(1_001)])   # the longest
    assert not use(2, 10, index=object())
    text = open(os.path.join(os.path.dirname(__file__), "..", "profiles", "bm25_groups.md"), encoding="utf-8").read()
    assert "GROUPS_RULE" in text and "bm25_groups_kernel" in text and "not decided" in text and "Not measured" in text


def test_the_field_map_is_built_once_per_field_and_rebuilt_when_the_records_change():
    r = _retriever()
    st = r._st()
    exprs = [f'source == "f{i % 4}.pdf"' for i in range(32)]
    r.batch_invoke(["q"] * 32, exprs=exprs)
    assert st["fields"].builds == 1                                           # 32 conditions: one walk, 32 look-ups
    r.batch_invoke(["q"] * 2, exprs=['page == 0', 'source == "f1.pdf" and page == 1'])
    assert st["fields"].builds == 2
    assert r._matching([("source", ["f1.pdf"])]).tolist() == [1, 5, 9] and st["fields"].builds == 2
    r.add_texts(["more"], [{"source": "f1.pdf"}])
    assert r._matching([("source", ["f1.pdf"])]).tolist() == [1, 5, 9, 12] and st["fields"].builds == 3
    assert r.delete(expr='pk == "id-5"').delete_count == 1 and st["fields"].builds == 4          # (the pk map; the delete drops both)
    assert r._matching([("source", ["f1.pdf"])]).tolist() == [1, 9, 12] and st["fields"].builds == 5
    # values that cannot be dictionary keys still match, as the walk matched them
    r.add_texts(["odd"], [{"tags": ["x", "y"]}])
    assert r._matching([("tags", ["x", "y"])]).tolist() == [13]
    assert r._matching([("row", [3, 4]), ("page", [0])]).tolist() == [4]
    assert r._matching([("source", [None])]).tolist() == [13]                                  # a document without the field holds None


def test_compact_and_load_drop_the_field_maps(librmu, tmp_path):
    from ragmeup_amd.bm25 import MI355XBM25Retriever
    r = MI355XBM25Retriever.from_texts([f"t{i}" for i in range(6)], metadatas=[{"s": i % 2} for i in range(6)], ids=[str(i) for i in range(6)])
    try:
        assert r._matching([("s", [1])]).tolist() == [1, 3, 5]
        r.delete(ids=["0", "1"])
        assert r._matching([("s", [1])]).tolist() == [3, 5]
        assert r.compact() == 2
        assert r._matching([("s", [1])]).tolist() == [1, 3]                                    # renumbered
        r.persist(str(tmp_path / "p"))
        back = MI355XBM25Retriever.load(str(tmp_path / "p"))
        try:
            assert back._matching([("s", [1])]).tolist() == [1, 3] and back._st()["fields"].builds == 1
        finally:
            back.vectorizer.close()
    finally:
        r.vectorizer.close()


# ---- ensemble and hybrid: the plurals reach both members ---------------------------------------------------------------------------------
class _Member:
    def __init__(self, tag):
        self.tag, self.seen = tag, []

    def batch_invoke(self, queries, filters=None, exprs=None):
        from ragmeup_amd._lc import Document
        self.seen.append((list(queries), filters, exprs))
        return [[Document(page_content=f"{self.tag}:{q}", metadata={})] for q in queries]


class _Plain:
    def batch_invoke(self, queries):
        return [[] for _ in queries]


class _InvokeOnly:
    def invoke(self, query):
        return []


def test_ensemble_and_hybrid_pass_the_plurals_to_both_members():
    from ragmeup_amd.ensemble import MI355XEnsembleRetriever
    from ragmeup_amd.hybrid import MI355XHybridRetriever
    exprs, flt = ['s == "a"', None], [None, {"s": "b"}]
    for make in (lambda a, b: MI355XEnsembleRetriever(retrievers=[a, b], weights=[0.5, 0.5]),
                 lambda a, b: MI355XHybridRetriever(sparse=a, dense=b, weights=[0.5, 0.5])):
        a, b = _Member("a"), _Member("b")
        ens = make(a, b)
        out = ens.batch_invoke(["x", "y"], exprs=exprs)
        assert a.seen == b.seen == [(["x", "y"], None, exprs)]
        assert [[d.page_content for d in row] for row in out] == [["a:x", "b:x"], ["a:y", "b:y"]]
        ens.batch_invoke(["x", "y"], filters=flt, exprs=exprs)
        assert a.seen[-1] == b.seen[-1] == (["x", "y"], flt, exprs)
        ens.batch_invoke(["x"])                                                # without a plural form: as ever
        assert a.seen[-1] == (["x"], None, None)
        for other in (_Plain(), _InvokeOnly()):
            bad = make(_Member("a"), other)
            with pytest.raises(ValueError):
                bad.batch_invoke(["x", "y"], exprs=exprs)
            with pytest.raises(ValueError):
                bad.batch_invoke(["x", "y"], filters=flt)
            if isinstance(other, _Plain):
                assert bad.batch_invoke(["x"]) == [[d] for d in bad.batch_invoke(["x"])[0]]      # and unfiltered it still serves


# ---- the code objects -------------------------------------------------------------------------------------------------------------------
def test_the_groups_kernel_is_in_the_library_without_scratch(tmp_path, librmu):
    """both instantiations of bm25_groups_kernel (k <= 64, k <= 112): no scratch, LDS <= 40960 (four workgroups per CU); the four kernels
    with the two older names are still four"""
    from ragmeup_amd import _native
    objdump, readelf = "/opt/rocm/lib/llvm/bin/llvm-objdump", "/opt/rocm/lib/llvm/bin/llvm-readelf"
    if not (os.path.exists(objdump) and os.path.exists(readelf)):
        pytest.skip("ROCm's llvm-objdump / llvm-readelf are not installed")
    so = tmp_path / "librmu.so"
    shutil.copy(os.path.join(os.path.dirname(_native.__file__), "lib", "librmu.so"), so)
    assert subprocess.run([objdump, "--offloading", str(so)], capture_output=True, text=True, cwd=tmp_path).returncode == 0
    scratch, lds = {}, {}
    for co in sorted(tmp_path.glob("librmu.so.*gfx950")):
        notes = subprocess.run([readelf, "--notes", str(co)], capture_output=True, text=True).stdout
        for lds_bytes, name, private in re.findall(
                r"\.group_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.name:\s+(\S+)\n\s+\.private_segment_fixed_size:\s+(\d+)", notes):
            if "bm25_" in name and "_kernel" in name:
                scratch[name], lds[name] = int(private), int(lds_bytes)
    groups = [n for n in scratch if "bm25_groups_kernel" in n]
    older = [n for n in scratch if "bm25_topk_kernel" in n or "bm25_masked_kernel" in n]
    assert len(groups) == 2 and len(older) == 4, sorted(scratch)
    assert all(scratch[n] == 0 and 0 < lds[n] <= 40960 for n in groups), (scratch, lds)
    assert {lds[n] for n in groups} == {lds[n] for n in older}                 # one body: the same accumulators and cursors
