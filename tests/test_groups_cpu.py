"""CPU: the grouped filtered search below the GPU -- rmu_index_search_groups' symbol, binding and every refusal that needs no device,
FlatIndex.search_groups' reordering (a pure function, against a brute-force numpy top-k behind a fake call that records what it is
given), and the store's per-query filters= / exprs= over the small exact numpy index of tests/test_subset_cpu.py."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests.test_subset_cpu import NumpyIndex, NumpyStore, _rows_where, _store

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- C-ABI ---------------------------------------------------------------------------------------------------------------------
def test_the_symbol_is_declared_exported_and_bound(librmu):
    from ragmeup_amd import _native
    header = open(os.path.join(ROOT, "include", "rmu.h")).read()
    assert re.search(r"\bint rmu_index_search_groups\(rmu_index_t\* idx, const float\* q, int64_t nq, int k, unsigned flags, int64_t row_base,\s*"
                     r"const int64_t\* rows, const int64_t\* list_ptr, int n_lists, const int32_t\* q_list,\s*"
                     r"float\* out_scores, int64_t\* out_rows, uint64_t hip_stream\);", header)
    assert hasattr(librmu, "rmu_index_search_groups")
    assert "rmu_index_search_groups" in _native.SYMBOLS
    assert len(librmu.rmu_index_search_groups.argtypes) == 13
    assert _native.MAX_QUERIES_PER_CALL == 8192


def _call(librmu, idx=None, nq=2, k=10, rows="ok", list_ptr="ok", n_lists=2, q_list="ok", q="ok", out="ok"):
    """rmu_index_search_groups with two small valid lists unless told otherwise (None = a NULL pointer); -> (return code, message).  The
    arrays stay alive until the call has returned."""
    a_rows = np.array([0, 1, 2, 1, 5], np.int64) if isinstance(rows, str) else rows
    a_ptr = np.array([0, 3, 5], np.int64) if isinstance(list_ptr, str) else list_ptr
    a_ql = np.zeros(max(int(nq), 1), np.int32) if isinstance(q_list, str) else q_list
    a_q = np.zeros((max(int(nq), 1), 384), np.float32) if isinstance(q, str) else q
    n_out = max(int(nq), 1) * max(int(k), 1)
    a_s, a_r = (np.zeros(n_out, np.float32), np.zeros(n_out, np.int64)) if isinstance(out, str) else (None, None)
    ptr = lambda a: None if a is None else a.ctypes.data
    rc = librmu.rmu_index_search_groups(idx, ptr(a_q), nq, k, 0, 0, ptr(a_rows), ptr(a_ptr), n_lists, ptr(a_ql), ptr(a_s), ptr(a_r), 0)
    return rc, librmu.rmu_last_error().decode()


def test_every_refusal_that_needs_no_device(librmu):
    for kw, word in ((dict(), "null index"),                                 # every other argument is fine: only the index is missing
                     (dict(q=None), "null pointer"), (dict(out=None), "null pointer"), (dict(list_ptr=None), "null pointer"),
                     (dict(q_list=None), "null pointer"), (dict(rows=None), "rows is null"),
                     (dict(k=113), "k must be in [1, 112]"), (dict(k=0), "k must be in [1, 112]"),
                     (dict(nq=8193), "nq must be in [1, 8192]"), (dict(nq=0), "nq must be in [1, 8192]"),
                     (dict(n_lists=0), "n_lists"),
                     (dict(list_ptr=np.array([1, 3, 5], np.int64)), "list_ptr[0]"),
                     (dict(list_ptr=np.array([0, 3, 2], np.int64)), "non-decreasing"),
                     (dict(list_ptr=np.array([0, 3, 2 ** 32], np.int64)), "2^32"),
                     (dict(q_list=np.array([1, 0], np.int32)), "q_list"),          # the queries of a list must be adjacent
                     (dict(q_list=np.array([0, 2], np.int32)), "q_list"), (dict(q_list=np.array([-1, 0], np.int32)), "q_list")):
        rc, msg = _call(librmu, **kw)
        assert rc == -1 and msg.startswith("rmu_index_search_groups: ") and word in msg, (kw, rc, msg)
    # all NULL, as tests/test_abi_cpu.py calls the other searches
    assert librmu.rmu_index_search_groups(None, None, 1, 10, 0, 0, None, None, 1, None, None, None, 0) == -1


def test_the_entry_point_follows_the_library_rules():
    """RMU_ENTRY() first, the index's shared lock, a drain at the end, and the pinned table documented in the header."""
    src = open(os.path.join(ROOT, "ragmeup_amd", "csrc", "rmu_api.hip")).read()
    m = re.search(r'^extern "C" int rmu_index_search_groups\([^;{]*\)\s*\{\n(.*?)^\}', src, flags=re.S | re.M)
    assert m
    body = m.group(1)
    assert "RMU_ENTRY();" in body.split("\n")[0]
    assert "std::shared_lock<std::shared_mutex> lk(idx->mu);" in body
    assert "hipStreamSynchronize(s)" in body and "hipDeviceSynchronize" not in body
    assert body.index("null index") < body.index("ensure_stream")           # every refusal above comes before the first HIP call
    header = open(os.path.join(ROOT, "include", "rmu.h")).read()
    doc = header[header.index("ONE LIST PER GROUP OF QUERIES"):header.index("int rmu_index_search_groups(")]
    assert "ALWAYS drains" in doc and "pinned" in doc and "Serves:" in doc and "8192" in doc


# ---- FlatIndex.search_groups: the reordering ---------------------------------------------------------------------------------------
def _brute(x, q, k, rows, row_base=0):
    s = q.astype(np.float64) @ x[rows].astype(np.float64).T
    out_s, out_r = np.full((q.shape[0], k), -np.inf, np.float32), np.full((q.shape[0], k), -1, np.int64)
    for i in range(q.shape[0]):
        order = np.lexsort((rows, -s[i]))[:k]
        out_s[i, :order.size], out_r[i, :order.size] = s[i, order], rows[order] + row_base
    return out_s, out_r


class FakeCall:
    """What FlatIndex._groups_call is to search_groups_blocks: checks the contract of the C call, answers by brute force, records."""

    def __init__(self, x):
        self.x, self.calls = x, []

    def __call__(self, q, k, rows, list_ptr, q_list, row_base):
        assert q.dtype == np.float32 and q.flags.c_contiguous and rows.dtype == np.int64 and list_ptr.dtype == np.int64 and q_list.dtype == np.int32
        assert list_ptr[0] == 0 and (np.diff(list_ptr) >= 0).all() and list_ptr[-1] == rows.shape[0]
        assert q_list.shape[0] == q.shape[0] and (np.diff(q_list) >= 0).all() and q_list.min() >= 0 and q_list.max() < list_ptr.shape[0] - 1
        self.calls.append((q.shape[0], list_ptr.shape[0] - 1, q_list.copy()))
        out_s, out_r = np.empty((q.shape[0], k), np.float32), np.empty((q.shape[0], k), np.int64)
        for i in range(q.shape[0]):
            out_s[i], out_r[i] = (a[0] for a in _brute(self.x, q[i:i + 1], k, rows[list_ptr[q_list[i]]:list_ptr[q_list[i] + 1]], row_base))
        return out_s, out_r


def test_search_groups_reorders_blocks_and_restores_the_callers_order():
    from ragmeup_amd.index import FlatIndex, search_groups_blocks
    import inspect
    assert list(inspect.signature(FlatIndex.search_groups).parameters)[1:] == ["q", "k", "lists", "q_list", "row_base"]
    rng = np.random.default_rng(5)
    x = rng.standard_normal((300, 16)).astype(np.float32)
    lists = [np.sort(rng.choice(300, n, replace=False)).astype(np.int64) for n in (40, 0, 7, 300, 1, 40)]
    lists[5] = lists[0].copy()                           # two identical lists
    q = rng.standard_normal((53, 16)).astype(np.float32)
    q_list = rng.integers(0, 5, 53)                      # any order; list 5 goes unused
    q_list[q_list == 1] = 5
    q_list[:3] = [4, 1, 0]
    for block in (8192, 16, 1):
        fake = FakeCall(x)
        s, r = search_groups_blocks(fake, q, 6, lists, q_list, row_base=1000, block=block)
        assert [c[0] for c in fake.calls] == [min(block, 53 - b) for b in range(0, 53, block)]
        for i in range(53):
            ws, wr = _brute(x, q[i:i + 1], 6, lists[q_list[i]], 1000)
            assert np.array_equal(r[i], wr[0]) and np.array_equal(s[i], ws[0]), (block, i)
        if block == 8192:                                # one call; it is given the range of lists its queries use
            assert fake.calls[0][1] == 6 and np.array_equal(fake.calls[0][2], np.sort(q_list))
    with pytest.raises(ValueError):
        search_groups_blocks(FakeCall(x), q, 6, lists, q_list[:-1])
    with pytest.raises(ValueError):
        search_groups_blocks(FakeCall(x), q, 6, lists, np.full(53, 6))


# ---- the store -----------------------------------------------------------------------------------------------------------------------
QUERIES = ["doc 7", "doc 100", "something else", "doc 9", "doc 33", "doc 7", "again"]
EXPRS = ['source == "a.pdf"', None, 'source == "b.pdf"', 'source == "a.pdf"', 'source == "nowhere.pdf"', None, 'source in ["c.pdf"] and lang == "en"']
FILTERS = [{"source": "a.pdf"}, None, {"source": "b.pdf"}, {"source": "a.pdf"}, {"lang": "fr"}, None, {"source": ["c.pdf"], "lang": "en"}]


def _contents(docs):
    return [d.page_content for d in docs]


@pytest.mark.parametrize("kwname,conds", [("exprs", EXPRS), ("filters", FILTERS)])
def test_per_query_conditions_equal_the_per_query_calls(kwname, conds):
    st = _store()
    one = "expr" if kwname == "exprs" else "filter"
    want_sim = [st.similarity_search_with_score(qy, k=5, **({} if c is None else {one: c})) for qy, c in zip(QUERIES, conds)]
    want_mmr = [st.max_marginal_relevance_search(qy, k=3, fetch_k=12, **({} if c is None else {one: c})) for qy, c in zip(QUERIES, conds)]
    assert want_sim[4] == [] and want_mmr[4] == [] and len(want_sim[0]) == 5
    st._index.calls.clear()
    got = st.similarity_search_with_score_batch(QUERIES, k=5, **{kwname: conds})
    # one unfiltered search for the None entries, then ONE call per distinct non-empty list (equal conditions share theirs; the empty
    # selection costs nothing)
    calls = st._index.calls
    assert len(calls) == 4 and calls[0] is None
    assert np.array_equal(calls[1], _rows_where(st, lambda m, pk: m["source"] == "a.pdf"))
    assert np.array_equal(calls[2], _rows_where(st, lambda m, pk: m["source"] == "b.pdf"))
    assert np.array_equal(calls[3], _rows_where(st, lambda m, pk: m["source"] == "c.pdf" and m["lang"] == "en"))
    assert len(got) == len(QUERIES)
    for g, w in zip(got, want_sim):
        assert _contents(d for d, _ in g) == _contents(d for d, _ in w) and [s for _, s in g] == [s for _, s in w]
    assert got[4] == []
    got = st.max_marginal_relevance_search_batch(QUERIES, k=3, fetch_k=12, **{kwname: conds})
    assert [_contents(g) for g in got] == [_contents(w) for w in want_mmr] and got[4] == []
    # the retriever forwards them
    got = st.as_retriever(search_kwargs={"k": 5}).batch_invoke(QUERIES, **{kwname: conds})
    assert [_contents(g) for g in got] == [_contents(d for d, _ in w) for w in want_sim]
    got = st.as_retriever(search_type="mmr", search_kwargs={"k": 3, "fetch_k": 12}).batch_invoke(QUERIES, **{kwname: conds})
    assert [_contents(g) for g in got] == [_contents(w) for w in want_mmr]


def test_all_none_entries_are_one_unfiltered_search_and_both_plurals_combine():
    st = _store()
    st._index.calls.clear()
    got = st.similarity_search_with_score_batch(QUERIES[:3], k=4, exprs=[None, None, None])
    assert len(st._index.calls) == 1 and st._index.calls[0] is None
    assert [_contents(d for d, _ in g) for g in got] == [_contents(d for d, _ in st.similarity_search_with_score(qy, k=4)) for qy in QUERIES[:3]]
    got = st.similarity_search_with_score_batch(QUERIES[:2], k=4, exprs=['lang == "en"', None], filters=[{"source": "a.pdf"}, {"source": "b.pdf"}])
    want = [st.similarity_search_with_score(QUERIES[0], k=4, expr='lang == "en"', filter={"source": "a.pdf"}),
            st.similarity_search_with_score(QUERIES[1], k=4, filter={"source": "b.pdf"})]
    assert [_contents(d for d, _ in g) for g in got] == [_contents(d for d, _ in w) for w in want]


def test_an_index_with_search_groups_gets_one_call_for_two_or_more_lists():
    class GroupsIndex(NumpyIndex):
        def search_groups(self, q, k, lists, q_list, row_base=0):
            self.group_calls.append(([np.array(l, copy=True) for l in lists], list(q_list)))
            out = [NumpyIndex.search(self, q[i:i + 1], k, row_base, rows=lists[g]) for i, g in enumerate(q_list)]
            return np.concatenate([o[0] for o in out]), np.concatenate([o[1] for o in out])

    class GroupsStore(NumpyStore):
        def _new_index(self, dim):
            idx = GroupsIndex(dim)
            idx.group_calls = []
            return idx

    st, plain = _store(cls=GroupsStore), _store()
    got = st.similarity_search_with_score_batch(QUERIES, k=5, exprs=EXPRS)
    want = plain.similarity_search_with_score_batch(QUERIES, k=5, exprs=EXPRS)
    assert [_contents(d for d, _ in g) for g in got] == [_contents(d for d, _ in w) for w in want]
    (lists, q_list), = st._index.group_calls                   # one grouped call: three distinct non-empty lists, the equal ones shared
    assert len(lists) == 3 and q_list == [0, 0, 1, 2]
    st._index.group_calls.clear()
    st._index.calls.clear()
    st.similarity_search_with_score_batch(QUERIES[:2], k=5, exprs=[EXPRS[0], EXPRS[0]])      # one distinct list: the ordinary subset call
    assert st._index.group_calls == [] and len(st._index.calls) == 1 and st._index.calls[0] is not None
    # lists that together hold more rows than the grouped call was measured ahead for (profiles/groups_search.md): the per-list loop
    assert GroupsStore.GROUPS_MAX_LIST_ROWS == 3_200_000
    GroupsStore.GROUPS_MAX_LIST_ROWS = 100               # (a class of this test's own)
    st._index.calls.clear()
    got = st.similarity_search_with_score_batch(QUERIES, k=5, exprs=EXPRS)
    assert st._index.group_calls == [] and len(st._index.calls) == 4
    assert [_contents(d for d, _ in g) for g in got] == [_contents(d for d, _ in w) for w in want]


def test_singular_and_plural_together_and_malformed_plurals_raise():
    st = _store()
    for kw in (dict(expr='source == "a.pdf"', exprs=EXPRS), dict(filter={"lang": "en"}, filters=FILTERS), dict(expr='lang == "en"', filters=FILTERS),
               dict(exprs=EXPRS[:3]), dict(filters="source"), dict(exprs=['page > 3'] + EXPRS[1:])):
        with pytest.raises(ValueError):
            st.similarity_search_with_score_batch(QUERIES, k=3, **kw)
        with pytest.raises(ValueError):
            st.max_marginal_relevance_search_batch(QUERIES, k=3, **kw)
    with pytest.raises(ValueError):                      # a list given as the SINGULAR expr= stays an error
        st.similarity_search_with_score_batch(QUERIES, k=3, expr=EXPRS)
    with pytest.raises(ValueError):
        st.as_retriever(search_kwargs={"k": 3, "expr": 'lang == "en"'}).batch_invoke(QUERIES, exprs=EXPRS)


# ---- the new kernels' resources ----------------------------------------------------------------------------------------------------
def test_the_grouped_kernels_use_no_scratch_and_keep_the_subset_family_apart(tmp_path, librmu):
    from ragmeup_amd import _native
    objdump = "/opt/rocm/lib/llvm/bin/llvm-objdump"
    readelf = "/opt/rocm/lib/llvm/bin/llvm-readelf"
    if not (os.path.exists(objdump) and os.path.exists(readelf)):
        pytest.skip("ROCm's llvm-objdump / llvm-readelf are not installed")
    so = tmp_path / "librmu.so"
    product = os.path.join(os.path.dirname(_native.__file__), "lib", "librmu.so")
    shutil.copy(product if os.path.exists(product) else _native.SO_PATH, so)
    r = subprocess.run([objdump, "--offloading", str(so)], capture_output=True, text=True, cwd=tmp_path)
    assert r.returncode == 0, r.stderr[-2000:]
    seen = {}
    for co in sorted(tmp_path.glob("librmu.so.*gfx950")):
        notes = subprocess.run([readelf, "--notes", str(co)], capture_output=True, text=True).stdout
        for name, scratch in re.findall(r"\.name:\s+(\S+)\n\s+\.private_segment_fixed_size:\s+(\d+)", notes):
            if "scan_groups_kernel" in name or "k_groups_" in name:
                seen[name] = int(scratch)
    scans = [n for n in seen if "scan_groups_kernel" in n]
    assert len(scans) == 9, sorted(seen)                 # the nine configurations of the gathered scan
    assert not any("scan_subset_kernel" in n for n in scans)
    assert any("k_groups_narrow" in n for n in seen) and any("k_groups_map" in n for n in seen)
    assert all(v == 0 for v in seen.values()), {n[:80]: v for n, v in seen.items() if v}
