"""CPU: the host half of the metadata columns (rmu_columns_create / append / size / compact never touch a GPU), every argument check of
rmu_columns_select and rmu_index_search_where (made before any HIP call), the Python binding, and the store's `device_fields` over a
CPU stand-in index: dictionaries, code rows in step with the index, demotion, and the host route wherever the device route cannot serve."""
import ctypes
import logging

import numpy as np
import pytest

from tests import where_cases as W
from tests.test_subset_cpu import HashEmbeddings, NumpyIndex, NumpyStore, _records

NEW = ("rmu_columns_create", "rmu_columns_free", "rmu_columns_size", "rmu_columns_append", "rmu_columns_compact", "rmu_columns_set_option",
       "rmu_columns_select", "rmu_index_search_where")


def _err(librmu):
    return librmu.rmu_last_error().decode()


def test_the_symbols_are_declared_exported_and_bound(librmu):
    import os
    from ragmeup_amd import _native as N
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "rmu.h")).read()
    for name in NEW:
        assert name + "(" in hdr and name in N.SYMBOLS and hasattr(librmu, name), name
    assert "RMU_COLUMNS_OPT_TILE_ROWS" in hdr and "typedef struct rmu_col_term" in hdr
    from ragmeup_amd import Columns, FlatIndex, MI355XVectorStore
    assert hasattr(FlatIndex, "search_where") and hasattr(Columns, "select")
    import inspect
    assert inspect.signature(MI355XVectorStore.__init__).parameters["device_fields"].default is None


def test_null_and_bad_arguments_return_minus_one_with_a_message(librmu):
    h = ctypes.c_void_p()
    for args in ((None, 2, 0), (ctypes.byref(h), 0, 0), (ctypes.byref(h), 9, 0), (ctypes.byref(h), 2, -1)):
        assert librmu.rmu_columns_create(*args) == -1 and "rmu_columns_create" in _err(librmu)
    n = ctypes.c_int64()
    assert librmu.rmu_columns_size(None, ctypes.byref(n), None) == -1 and _err(librmu)
    assert librmu.rmu_columns_append(None, None, 0, None) == -1 and _err(librmu)
    assert librmu.rmu_columns_compact(None, None, 0, None) == -1 and _err(librmu)
    assert librmu.rmu_columns_set_option(None, 1, 0) == -1 and _err(librmu)
    assert librmu.rmu_columns_select(None, None, 0, None, None, 1, 0, None, 0, None, 0) == -1 and "null" in _err(librmu)
    assert librmu.rmu_index_search_where(None, None, None, 1, 5, 0, 0, None, 0, None, None, 1, None, None, None, 0) == -1 and "null" in _err(librmu)
    assert librmu.rmu_columns_free(None) == 0
    assert librmu.rmu_columns_create(ctypes.byref(h), 2, 0) == 0
    try:
        assert librmu.rmu_columns_append(h, None, 3, None) == -1
        for bad in (-1, 32, 63, 100, 32768):
            assert librmu.rmu_columns_set_option(h, 1, bad) == -1 and "power of two" in _err(librmu)
        assert librmu.rmu_columns_set_option(h, 2, 64) == -1
        for ok in (64, 16384, 0):
            assert librmu.rmu_columns_set_option(h, 1, ok) == 0
        lp = (ctypes.c_int64 * 2)()
        assert librmu.rmu_columns_select(h, None, 0, None, None, 1, 0, None, 0, lp, 0) == -1           # no terms
        assert librmu.rmu_columns_select(h, None, 0, None, None, 1, 4, None, 0, lp, 0) == -1 and "flag" in _err(librmu)
    finally:
        assert librmu.rmu_columns_free(h) == 0


def test_append_size_compact_on_the_host(librmu):
    from ragmeup_amd import Columns
    from ragmeup_amd import _native as N
    codes = W.make_codes(257)
    c = Columns(W.N_FIELDS)
    assert len(c) == 0
    assert c.append(codes[:100]) == 0 and c.append(codes[100:]) == 100 and len(c) == 257
    assert c.append(np.zeros((0, 2), np.int32)) == 257 and len(c) == 257
    bad = codes[:5].copy()
    bad[3, 1] = -1
    with pytest.raises(N.RmuError) as e:
        c.append(bad)
    assert e.value.code == -1 and "row 3, field 1" in str(e.value) and len(c) == 257      # refused, nothing changed
    with pytest.raises(ValueError):
        c.append(np.zeros((4, 3), np.int32))
    dead = [0, 5, 6, 100, 256]
    m, after = W.compact_reference(codes, dead)
    with pytest.raises(N.RmuError) as e:
        c.compact(m[:-1])                                    # map_len too short
    assert e.value.code == -1 and len(c) == 257
    wrong = m.copy()
    wrong[1], wrong[2] = m[2], m[1]
    with pytest.raises(N.RmuError):
        c.compact(wrong)                                     # not the order-keeping map of a compaction
    assert len(c) == 257
    assert c.compact(np.concatenate([m, [-1, -1]])) == 252 == len(c) == after.shape[0]      # (map_len >= rows)
    assert c.compact(np.arange(252)) == 252                  # nothing dropped: nothing changes
    assert c.append(after[:3]) == 252
    nf = ctypes.c_int()
    n = ctypes.c_int64()
    assert librmu.rmu_columns_size(c._h, ctypes.byref(n), ctypes.byref(nf)) == 0 and (n.value, nf.value) == (255, 2)
    c.close()
    c.close()


def _select_rc(librmu, c, sels, dedup=True):
    from ragmeup_amd.index import flatten_selections
    if dedup:
        terms, codes, ptr = flatten_selections(sels)
    else:
        terms, codes, ptr = sels
    lp = np.zeros(len(ptr), np.int64)
    rc = librmu.rmu_columns_select(c._h, terms.ctypes.data, terms.shape[0], codes.ctypes.data, ptr.ctypes.data, len(ptr) - 1, 0, None, 0,
                                   lp.ctypes.data, 0)
    return rc, _err(librmu)


def _raw(sel_terms, codes, ptr):
    return (np.asarray(sel_terms, np.int32).reshape(-1, 3), np.asarray(codes, np.int32), np.asarray(ptr, np.int32))


def test_selection_errors_are_refused_before_any_hip_call_and_name_the_selection(librmu):
    """The handle holds rows, so a call that passed the checks would go on to the device: on this GPU-less box every case must come back
    RMU_E_INVALID (-1), never a HIP error (-2)."""
    from ragmeup_amd import Columns
    c = Columns(2)
    c.append(W.make_codes(65))
    ok = [(0, 0, 1)]
    cases = {
        "unsorted codes": _raw(ok + [(1, 1, 4)], [3, 5, 9, 7], [0, 1, 2]),
        "a duplicate code": _raw(ok + [(1, 1, 4)], [3, 5, 5, 7], [0, 1, 2]),
        "a negative code": _raw(ok + [(1, 1, 3)], [3, -1, 7], [0, 1, 2]),
        "field out of range": _raw(ok + [(2, 1, 2)], [3, 5], [0, 1, 2]),
        "field negative": _raw(ok + [(-1, 1, 2)], [3, 5], [0, 1, 2]),
        "5 terms": _raw(ok + [(0, 0, 1)] * 5, [3], [0, 1, 6]),
        "no term": _raw(ok + [(0, 0, 1)], [3], [0, 1, 1, 2]),
        "1025 codes": _raw(ok + [(1, 1, 1026)], [3] + list(range(1025)), [0, 1, 2]),
        "1025 codes over two terms": _raw(ok + [(1, 1, 1001), (0, 1001, 1026)], [3] + list(range(1000)) + list(range(25)), [0, 1, 3]),
    }
    for what, raw in cases.items():
        rc, msg = _select_rc(librmu, c, raw, dedup=False)
        assert rc == -1 and "selection 1" in msg, (what, rc, msg)             # (selection 0 is fine in every case)
    # exactly 1 024 codes and 4 terms pass the checks: on a GPU-less box the call then fails in HIP (-2 / -3), with a GPU it succeeds
    rc, msg = _select_rc(librmu, c, _raw([(1, 0, 1024)], list(range(1024)), [0, 1]), dedup=False)
    assert rc != -1, msg
    for n_sel in (0, 8193):
        ptr = np.zeros(n_sel + 1, np.int32)
        lp = np.zeros(n_sel + 1, np.int64)
        t = np.zeros((1, 3), np.int32)
        assert librmu.rmu_columns_select(c._h, t.ctypes.data, 0, None, ptr.ctypes.data, n_sel, 0, None, 0, lp.ctypes.data, 0) == -1
        assert "n_sel" in _err(librmu)
    # sel_ptr that does not cover the terms
    rc, msg = _select_rc(librmu, c, _raw(ok * 2, [3], [0, 1]), dedup=False)
    assert rc == -1 and "sel_ptr" in msg


def test_search_where_checks_q_sel_and_the_limits_before_it_looks_at_the_index(librmu):
    """An index cannot be created without a GPU, and the contract puts these checks in front of everything that reads it: the handle passed
    here is a block of zeros that is never dereferenced.  ("out of step" and the wide index need a real one: tests/test_where_gpu.py.)"""
    from ragmeup_amd import Columns
    fake = ctypes.create_string_buffer(4096)
    c = Columns(2)
    terms, codes, ptr = _raw([(0, 0, 1), (1, 1, 2)], [3, 5], [0, 1, 2])
    q = np.zeros((3, 64), np.float32)
    s = np.zeros((3, 5), np.float32)
    r = np.zeros((3, 5), np.int64)

    def call(q_sel, nq=3, k=5, n_sel=2, flags=0):
        qs = np.asarray(q_sel, np.int32)
        rc = librmu.rmu_index_search_where(ctypes.addressof(fake), c._h, q.ctypes.data, nq, k, flags, 0, terms.ctypes.data, terms.shape[0],
                                           codes.ctypes.data, ptr.ctypes.data, n_sel, qs.ctypes.data, s.ctypes.data, r.ctypes.data, 0)
        return rc, _err(librmu)
    rc, msg = call([1, 0, 1])
    assert rc == -1 and "q_sel" in msg and "entry 1" in msg                    # decreasing
    rc, msg = call([0, 1, 2])
    assert rc == -1 and "q_sel" in msg and "selection 2" in msg                # out of range
    rc, msg = call([-1, 0, 1])
    assert rc == -1 and "q_sel" in msg
    assert call([0, 0, 1], k=0)[0] == -1 and call([0, 0, 1], k=113)[0] == -1
    assert call([0, 0, 1], nq=0)[0] == -1 and call([0, 0, 1], nq=8193)[0] == -1
    assert call([0, 0, 1], flags=8)[0] == -1
    rc, msg = call([0, 0, 1], n_sel=0)
    assert rc == -1 and "n_sel" in msg
    terms[1, 0] = 2                                                            # a selection error through this entry point
    rc, msg = call([0, 0, 1])
    assert rc == -1 and "selection 1" in msg and "rmu_index_search_where" in msg


def test_the_binding_deduplicates_and_sorts_the_codes():
    from ragmeup_amd.index import flatten_selections
    terms, codes, ptr = flatten_selections([[(1, [9, 3, 3, 7]), (0, [])], [(0, [2])]])
    assert terms.tolist() == [[1, 0, 3], [0, 3, 3], [0, 3, 4]] and codes.tolist() == [3, 7, 9, 2] and ptr.tolist() == [0, 2, 3]
    assert terms.dtype == codes.dtype == ptr.dtype == np.int32
    with pytest.raises(ValueError):
        flatten_selections([[(0, [-1])]])


def test_the_selection_kernels_use_no_scratch(tmp_path, librmu):
    """The way tests/test_wide_cpu.py reads it: the code objects inside librmu.so carry every kernel's resources."""
    import os
    import re
    import shutil
    import subprocess
    from ragmeup_amd import _native
    objdump, readelf = "/opt/rocm/lib/llvm/bin/llvm-objdump", "/opt/rocm/lib/llvm/bin/llvm-readelf"
    if not (os.path.exists(objdump) and os.path.exists(readelf)):
        pytest.skip("ROCm's llvm-objdump / llvm-readelf are not installed")
    so = tmp_path / "librmu.so"
    product = os.path.join(os.path.dirname(_native.__file__), "lib", "librmu.so")
    shutil.copy(product if os.path.exists(product) else _native.SO_PATH, so)
    assert subprocess.run([objdump, "--offloading", str(so)], capture_output=True, text=True, cwd=tmp_path).returncode == 0
    found = {}
    for co in sorted(tmp_path.glob("librmu.so.*gfx950")):
        notes = subprocess.run([readelf, "--notes", str(co)], capture_output=True, text=True).stdout
        for name, scratch in re.findall(r"\.name:\s+(\S+)\n\s+\.private_segment_fixed_size:\s+(\d+)", notes):
            if re.search(r"col_(count|scan|write)_kernel", name):
                found[name] = int(scratch)
    assert len(found) == 4, found                            # count, write, and the scan over u32 and over int64
    assert set(found.values()) == {0}, found


# ---- the store over a CPU stand-in index ----------------------------------------------------------------------------------------------
class SavingIndex(NumpyIndex):
    """NumpyIndex + the save / load a store's persist() and load() call."""

    def save(self, path):
        with open(path, "wb") as f:
            np.savez(f, x=self.x, alive=self.alive)

    @classmethod
    def load(cls, path):
        with open(path, "rb") as f:
            z = np.load(f)
            self = cls(z["x"].shape[1])
            self.x, self.alive = z["x"], z["alive"]
        return self


class HostStore(NumpyStore):
    def _new_index(self, dim):
        return SavingIndex(dim)

    def _open_index(self, path):
        return SavingIndex.load(path)


class WhereIndex(SavingIndex):
    """NumpyIndex + search_where in numpy over a stand-in for the code rows: what the device route must return, and a record of its calls."""

    def __init__(self, dim):
        super().__init__(dim)
        self.where_calls = []
        self.before_where = None                            # a hook the tests use to let an insert run between the store's check and the call

    def search_where(self, q, k, columns, selections, q_sel, row_base=0):
        q = np.asarray(q, np.float32).reshape(-1, self.dim)
        self.where_calls.append((list(selections), list(q_sel)))
        if self.before_where is not None:
            hook, self.before_where = self.before_where, None
            hook()
        codes = columns.codes()
        if codes.shape[0] != len(self):                     # the library's own refusal (rmu_index_search_where)
            from ragmeup_amd import _native as N
            raise N.RmuError(-1, "rmu_index_search_where", f"rmu_index_search_where: the columns ({codes.shape[0]} rows) and the index "
                                                           f"({len(self)} rows) are out of step")
        out_s = np.full((q.shape[0], k), -np.inf, np.float32)
        out_r = np.full((q.shape[0], k), -1, np.int64)
        n_calls = len(self.calls)
        for i, g in enumerate(q_sel):
            out_s[i], out_r[i] = (a[0] for a in NumpyIndex.search(self, q[i:i + 1], k, row_base, rows=W.reference(codes, selections[g])))
        del self.calls[n_calls:]
        return out_s, out_r


class HostColumns:
    """The host half of ragmeup_amd.Columns (the real one, so append / compact run the library) + a numpy mirror the stand-in index reads."""

    def __init__(self, n_fields):
        from ragmeup_amd import Columns
        self.real = Columns(n_fields)
        self.rows = np.zeros((0, n_fields), np.int32)

    def __len__(self):
        assert len(self.real) == self.rows.shape[0]
        return len(self.real)

    def append(self, codes):
        self.rows = np.concatenate([self.rows, np.asarray(codes, np.int32)])
        return self.real.append(codes)

    def compact(self, m):
        m = np.asarray(m)
        self.rows = self.rows[m[:self.rows.shape[0]] >= 0]
        return self.real.compact(m)

    def codes(self):
        return self.rows

    def close(self):
        self.real.close()


class WhereStore(NumpyStore):
    def _new_index(self, dim):
        return WhereIndex(dim)

    def _open_index(self, path):
        return WhereIndex.load(path)

    def _new_columns(self, n_fields):
        return HostColumns(n_fields)


def _pair(cls_dev=WhereStore, fields=("source", "lang"), n=240):
    texts, metas, ids = _records(n)
    host = NumpyStore(embeddings=HashEmbeddings(), collection_name="where-host", auto_persist=False)
    dev = cls_dev(embeddings=HashEmbeddings(), collection_name="where-dev", auto_persist=False, device_fields=fields)
    for st in (host, dev):
        st.add_texts(texts[:150], metas[:150], ids=ids[:150])
        st.add_texts(texts[150:], metas[150:], ids=ids[150:])
    return host, dev


EXPRS = ['source == "a.pdf"', None, 'source == "b.pdf" and lang == "nl"', 'source == "a.pdf"', 'source == "nowhere.pdf"',
         'source in ["a.pdf", "c.pdf"] and lang == "en"', 'page == 3', 'source == "a.pdf" and page == 3', 'pk == "pk007"']
QUERIES = ["query %d" % i for i in range(len(EXPRS))]


def _answers(st):
    docs = lambda ds: [(d.page_content, d.metadata) for d in ds]
    batch = st.similarity_search_with_score_batch(QUERIES, k=6, exprs=EXPRS)
    out = [[(d.page_content, d.metadata, s) for d, s in g] for g in batch]
    out.append([docs(g) for g in st.max_marginal_relevance_search_batch(QUERIES, k=4, fetch_k=20, exprs=EXPRS)])
    out.append(docs(st.similarity_search(QUERIES[0], k=5, expr=EXPRS[5])))
    out.append(docs(st.max_marginal_relevance_search(QUERIES[1], k=3, fetch_k=12, filter={"source": ["a.pdf", "b.pdf"], "lang": "nl"})))
    out.append(docs(st.similarity_search(QUERIES[2], k=5, expr='lang == "fr"')))
    out.append(docs(st.similarity_search(QUERIES[3], k=5, expr='lang == "nl"')))
    return out


def _decoded(st):
    """the code rows decoded through the dictionaries == the records' values, for every row that has a live record"""
    inv = [{c: v for v, c in d.items()} for d in st._dev_codes]
    rows = st._columns.codes()
    assert rows.shape[0] == len(st._index) == len(st._metas)
    for field, j in st._device_fields.items():
        if field in st._dev_demoted:
            continue
        for r in range(rows.shape[0]):
            if st._alive[r]:
                assert inv[j][int(rows[r, j])] == st._metas[r].get(field), (field, r)


def test_default_store_has_no_columns_and_device_fields_are_validated():
    st = NumpyStore(embeddings=HashEmbeddings(), collection_name="where-none", auto_persist=False)
    st.add_texts(["a", "b"], [{"source": "x"}, {"source": "y"}])
    assert st._columns is None and st._device_fields == {}
    for bad in ((), ("pk",), ("a", "a"), tuple("abcdefghi")):
        with pytest.raises(ValueError):
            NumpyStore(embeddings=HashEmbeddings(), collection_name="where-bad", auto_persist=False, device_fields=bad)


def test_an_index_without_search_where_takes_the_host_route_with_the_same_results():
    host, dev = _pair(cls_dev=NumpyStore)                   # device_fields set, NumpyIndex has no search_where; the real Columns (host half)
    assert len(dev._columns) == len(dev._index) == 240 and not hasattr(dev._index, "search_where")
    assert _answers(dev) == _answers(host)
    assert dev._field_map_builds == host._field_map_builds > 0


def test_the_device_route_gives_the_host_routes_results_and_builds_no_field_map():
    host, dev = _pair()
    want = _answers(host)
    assert _answers(dev) == want
    # page and pk are no device fields: those conditions (and the mixed one) took the host route -- and only those
    # (the mixed one needs the host's map of `source` as well: source, page, pk)
    assert dev._field_map_builds == 3 and host._field_map_builds == 4
    sels, q_sel = dev._index.where_calls[0]
    assert len(sels) == 3 and sorted(q_sel) == [0, 0, 1, 2]                   # a.pdf twice, b.pdf & nl, in [..] & en; "nowhere.pdf": no launch
    src, lang = dev._dev_codes
    assert sels[0] == [(0, [src["a.pdf"]])] and sels[1] == [(0, [src["b.pdf"]]), (1, [lang["nl"]])]
    assert sels[2] == [(0, sorted([src["a.pdf"], src["c.pdf"]])), (1, [lang["en"]])]
    _decoded(dev)


def test_codes_stay_stable_and_in_step_across_add_upsert_delete_compact_and_load(tmp_path):
    texts, metas, ids = _records()
    host = HostStore(embeddings=HashEmbeddings(), collection_name="h", auto_persist=False, connection=str(tmp_path / "host.db"))
    dev = WhereStore(embeddings=HashEmbeddings(), collection_name="d", auto_persist=False, connection=str(tmp_path / "dev.db"),
                     device_fields=("source", "lang"))
    both = (host, dev)
    for st in both:
        st.add_texts(texts, metas, ids=ids)
    first = [dict(d) for d in dev._dev_codes]
    builds = dev._field_map_builds

    def check():
        _decoded(dev)
        assert all(dev._dev_codes[j][v] == c for j in range(2) for v, c in first[j].items())      # a value keeps its code
        return _answers(dev) == _answers(host)
    assert check()
    for st in both:                                         # upsert: 30 records move to a new source, 5 lose their lang
        st.add_texts(texts[10:40], [dict(m, source="new.pdf") for m in metas[10:40]], ids=ids[10:40])
        st.add_texts(texts[50:55], [{"source": "a.pdf", "page": 1} for _ in range(5)], ids=ids[50:55])
    assert len(dev._columns) == len(dev._index) == 275 and dev._dev_codes[0]["new.pdf"] == 3 and check()
    for st in both:
        assert st.delete(expr='source == "c.pdf"').delete_count > 0
    assert check()
    for st in both:
        assert st.compact() > 0
    assert len(dev._columns) == len(dev._index) == sum(dev._alive) and check()
    for st in both:
        st.add_texts(["late one", "late two"], [{"source": "late.pdf", "lang": "en"}, {"source": "a.pdf", "lang": "xx"}], ids=["l1", "l2"])
    assert check()
    for st in both:
        assert st.persist() and st.load()
    assert len(dev._columns) == len(dev._index) and check()
    fresh = WhereStore(embeddings=HashEmbeddings(), collection_name="d", auto_persist=False, connection=str(tmp_path / "dev.db"),
                       device_fields=("source", "lang"))
    assert fresh.load() and len(fresh._columns) == len(fresh._index) == len(dev._index)
    _decoded(fresh)
    assert _answers(fresh) == _answers(host)
    # only the conditions that name page / pk (source, page, pk: one map each) walked the records of the reloaded store
    assert fresh._field_map_builds == 3


def test_an_unhashable_value_demotes_the_field_once(caplog):
    host, dev = _pair()
    with caplog.at_level(logging.WARNING, logger="ragmeup_amd"):
        for st in (host, dev):
            st.add_texts(["odd one"], [{"source": ["x", "y"], "lang": "en"}], ids=["odd"])
            st.add_texts(["odd two"], [{"source": {"k": 1}, "lang": "nl"}], ids=["odd2"])
    assert dev._dev_demoted == {"source"} and len(dev._columns) == len(dev._index) == 242
    assert sum("unhashable" in r.getMessage() for r in caplog.records) == 1
    calls = len(dev._index.where_calls)
    assert _answers(dev) == _answers(host)
    # `lang` alone is still the device route's; everything that names `source` is the host's
    assert all(all(f == 1 for f, _ in sel) for sels, _ in dev._index.where_calls[calls:] for sel in sels)
    assert len(dev._index.where_calls) > calls
    docs = lambda ds: [(d.page_content, d.metadata) for d in ds]
    assert docs(dev.similarity_search("q", k=3, filter={"source": [["x", "y"]]})) == docs(host.similarity_search("q", k=3, filter={"source": [["x", "y"]]}))


class LaggingStore(WhereStore):
    """While `lag` is set an insert stops where a concurrent search can see it in the real store: records written, rows in the index, code rows
    not appended yet."""
    lag = False

    def _columns_follow(self):
        if not self.lag:
            super()._columns_follow()


def test_an_insert_between_the_stores_check_and_the_call_falls_back_to_the_host_route():
    """Searches run without the writer lock and an insert appends to the index before the code rows, so a search can pass the store's own
    comparison and still be refused as "out of step" by the library.  The interleaving is forced: the stand-in index runs the insert's first
    half at the top of search_where and then refuses as the library does.  The search must answer -- through the host route -- what the
    store without device fields answers for the same records, and the device route must be back once the code rows have followed."""
    host, dev = _pair(cls_dev=LaggingStore)
    new = (["slipped in %d" % i for i in range(3)], [{"source": "a.pdf", "lang": "nl"}, {"source": "z.pdf", "lang": "en"}, {"source": "b.pdf"}],
           ["new0", "new1", "new2"])
    host.add_texts(*new)

    def half_an_insert():
        dev.lag = True
        dev.add_texts(*new)
        dev.lag = False
    for entry in ("batch", "single"):
        if entry == "single":
            host.add_texts(["one more"], [{"source": "a.pdf", "lang": "en"}], ids=["new3"])
            new = (["one more"], [{"source": "a.pdf", "lang": "en"}], ["new3"])
        dev._index.before_where = half_an_insert
        calls, builds = len(dev._index.where_calls), dev._field_map_builds
        if entry == "batch":
            got = dev.similarity_search_with_score_batch(QUERIES, k=6, exprs=EXPRS)
            want = host.similarity_search_with_score_batch(QUERIES, k=6, exprs=EXPRS)
        else:
            got = [dev.similarity_search_with_score(QUERIES[0], k=6, expr=EXPRS[0])]
            want = [host.similarity_search_with_score(QUERIES[0], k=6, expr=EXPRS[0])]
        assert dev._index.before_where is None and len(dev._index.where_calls) == calls + 1       # the device route was tried, once
        assert len(dev._columns) == len(dev._index) - len(new[0])                                # ... and met the index one insert ahead
        assert dev._field_map_builds > builds                                                    # the host route answered
        assert [[(d.page_content, d.metadata, s) for d, s in g] for g in got] == [[(d.page_content, d.metadata, s) for d, s in g] for g in want]
        dev._columns_follow()                                                                    # the insert's second half
        assert len(dev._columns) == len(dev._index)
    calls = len(dev._index.where_calls)
    assert _answers(dev) == _answers(host) and len(dev._index.where_calls) > calls
    _decoded(dev)


def test_other_refusals_of_the_device_route_are_raised():
    from ragmeup_amd import _native as N
    _, dev = _pair()

    def broken(*a, **kw):
        raise N.RmuError(-2, "rmu_index_search_where", "hipErrorUnknown")
    dev._index.search_where = broken
    with pytest.raises(N.RmuError):
        dev.similarity_search("q", k=3, expr='source == "a.pdf"')
