"""CPU: the filtered search below the GPU -- the C-ABI symbol and its binding, argument validation before any HIP call, the expression
parser shared by delete() and the searches, the per-field row maps (built once, dropped when records change), every store entry point
handing the resolved rows to its index (a small exact numpy index of this file's own), and the new kernels' resources."""
import ctypes
import hashlib
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from ragmeup_amd import records
from ragmeup_amd.vectorstore import MI355XVectorStore

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- C-ABI ---------------------------------------------------------------------------------------------------------------------
def test_the_symbol_is_exported_and_bound(librmu):
    from ragmeup_amd import _native
    assert hasattr(librmu, "rmu_index_search_subset")
    assert "rmu_index_search_subset" in _native.SYMBOLS
    assert len(librmu.rmu_index_search_subset.argtypes) == 11
    header = open(os.path.join(ROOT, "include", "rmu.h")).read()
    m = re.search(r"#define RMU_F_ROWS_DEVICE (\d+)u", header)
    assert m and int(m.group(1)) == _native.F_ROWS_DEVICE == 8
    assert "rmu_index_search_subset" in header and "filter=" in header and "expr=" in header      # names the reference call it serves


def test_invalid_arguments_fail_without_a_gpu(librmu):
    rows = np.arange(4, dtype=np.int64)
    q = np.zeros(384, np.float32)
    s, r = np.zeros(10, np.float32), np.zeros(10, np.int64)
    assert librmu.rmu_index_search_subset(None, q.ctypes.data, 1, 10, 0, 0, rows.ctypes.data, 4, s.ctypes.data, r.ctypes.data, 0) == -1
    assert b"rmu_index_search_subset" in librmu.rmu_last_error()
    assert librmu.rmu_index_search_subset(None, None, 1, 10, 0, 0, None, 0, None, None, 0) == -1


def test_flatindex_search_takes_rows():
    import inspect
    from ragmeup_amd.index import FlatIndex
    sig = inspect.signature(FlatIndex.search)
    assert list(sig.parameters)[1:] == ["q", "k", "row_base", "stream", "out", "rows"]
    assert sig.parameters["rows"].default is None


# ---- the expression parser -----------------------------------------------------------------------------------------------------
def test_expression_parser_accepted_forms():
    P = records.parse_expr
    assert P('source == "a.pdf"') == [("source", ["a.pdf"])]
    assert P("  source=='a.pdf'  ") == [("source", ["a.pdf"])]
    assert P('source in ["a.pdf", \'b.pdf\']') == [("source", ["a.pdf", "b.pdf"])]
    assert P('source == "a.pdf" and lang == "en"') == [("source", ["a.pdf"]), ("lang", ["en"])]
    assert P('source in ["a", "b"] && lang in ["en"] and page == 3') == [("source", ["a", "b"]), ("lang", ["en"]), ("page", [3])]
    assert P("score == 2.5") == [("score", [2.5])]
    assert P('pk == "id-1"') == [("pk", ["id-1"])]
    # what delete() always took keeps its meaning: one equality whose value holds quotes or the word `and`
    assert P('source == "/data/it\'s here.pdf"') == [("source", ["/data/it's here.pdf"])]
    assert P('source == "the "quoted" name.pdf"') == [("source", ['the "quoted" name.pdf'])]
    assert P('source == "rock and roll.pdf"') == [("source", ["rock and roll.pdf"])]
    C = records.conditions
    assert C(None, None) is None
    assert C(None, {"source": "a", "lang": ["en", "nl"]}) == [("source", ["a"]), ("lang", ["en", "nl"])]
    assert C('page == 1', {"source": "a"}) == [("source", ["a"]), ("page", [1])]


@pytest.mark.parametrize("bad", ['source = "a.pdf"', "source == a.pdf", 'source == "a.pdf" and', 'page > 3', 'source == "a" or lang == "en"',
                                 "", "   ", "source in []", 'source in ["a"', 'source in "a"', '== "a"', 'source == "a" lang == "b"',
                                 'source != "a"', 'source like "a%"'])
def test_expression_parser_rejects_what_it_does_not_understand(bad):
    with pytest.raises(ValueError):
        records.conditions(bad, None)


def test_filter_must_be_a_dict():
    with pytest.raises(ValueError):
        records.conditions(None, "source == 'a'")
    with pytest.raises(ValueError):
        records.conditions(["source"], None)


# ---- a small exact index of this file's own -------------------------------------------------------------------------------------
class NumpyIndex:
    """search(q, k, row_base=0, rows=None) exactly in numpy (inner product, fp64; order: score, then lower row); records every call."""

    def __init__(self, dim):
        self.dim, self.x, self.alive, self.calls = dim, np.zeros((0, dim), np.float32), np.zeros(0, bool), []

    def __len__(self):
        return self.x.shape[0]

    def add(self, v):
        first = self.x.shape[0]
        self.x = np.concatenate([self.x, np.asarray(v, np.float32)])
        self.alive = np.concatenate([self.alive, np.ones(len(v), bool)])
        return first

    def remove_rows(self, rows):
        n = int(self.alive[list(rows)].sum()); self.alive[list(rows)] = False; return n

    def compact(self):
        m = np.where(self.alive, np.cumsum(self.alive) - 1, -1).astype(np.int64)
        self.x, self.alive = self.x[self.alive], np.ones(int(self.alive.sum()), bool)
        return m

    def get_rows(self, rows):
        return self.x[list(rows)]

    def search(self, q, k, row_base=0, rows=None):
        q = np.asarray(q, np.float64).reshape(-1, self.dim)
        self.calls.append(None if rows is None else np.array(rows, copy=True))
        cand = np.arange(len(self)) if rows is None else np.asarray(rows, np.int64)
        if rows is not None:
            assert cand.dtype == np.int64 and cand.ndim == 1 and (np.diff(cand) > 0).all() and (cand >= 0).all() and (cand < len(self)).all()
        cand = cand[self.alive[cand]]
        out_s = np.full((q.shape[0], k), -np.inf, np.float32)
        out_r = np.full((q.shape[0], k), -1, np.int64)
        if cand.size:
            s = q @ self.x[cand].astype(np.float64).T
            for i in range(q.shape[0]):
                order = np.lexsort((cand, -s[i]))[:k]
                out_s[i, :order.size] = s[i, order]
                out_r[i, :order.size] = cand[order] + row_base
        return out_s, out_r


class NumpyStore(MI355XVectorStore):
    def _new_index(self, dim):
        return NumpyIndex(dim)

    def _embed_docs_for_index(self, texts):
        return self._embed_docs(texts)


class HashEmbeddings:
    def embed_documents(self, texts):
        out = []
        for t in texts:
            v = np.random.default_rng(int(hashlib.md5(t.encode()).hexdigest()[:8], 16)).standard_normal(48)
            out.append((v / np.linalg.norm(v)).tolist())
        return out

    def embed_query(self, t):
        return self.embed_documents([t])[0]


def _records(n=240):
    texts = ["doc %d" % i for i in range(n)]
    metas = [{"source": "%s.pdf" % "abc"[i % 3], "lang": ("en", "nl")[(i // 3) % 2], "page": i % 5} for i in range(n)]
    return texts, metas, ["pk%03d" % i for i in range(n)]


def _store(keep=None, cls=NumpyStore):
    texts, metas, ids = _records()
    sel = [i for i in range(len(texts)) if keep is None or keep(metas[i], ids[i])]
    st = cls(embeddings=HashEmbeddings(), collection_name="subset-cpu", auto_persist=False)
    st.add_texts([texts[i] for i in sel], [metas[i] for i in sel], ids=[ids[i] for i in sel])
    return st


def _rows_where(st, keep):
    return np.array([r for r in range(len(st._alive)) if st._alive[r] and keep(st._metas[r], st._pks[r])], np.int64)


def test_field_maps_are_built_once_and_rebuilt_when_records_change():
    st = _store()
    a_pdf = lambda m, pk: m["source"] == "a.pdf"
    assert st._field_map_builds == 0                     # nothing is built for unfiltered queries
    st.similarity_search("doc 1", k=3)
    assert st._field_map_builds == 0
    for _ in range(5):
        st.similarity_search("doc 1", k=3, expr='source == "a.pdf"')
    assert st._field_map_builds == 1                     # one walk over the records, not one per query
    assert np.array_equal(st._index.calls[-1], _rows_where(st, a_pdf))
    st.similarity_search("doc 1", k=3, filter={"source": "b.pdf", "lang": "en"})
    st.similarity_search("doc 2", k=3, filter={"lang": "nl"})
    assert st._field_map_builds == 2                     # `source` was there already; `lang` is new
    # add
    st.add_texts(["new a"], [{"source": "a.pdf", "lang": "en", "page": 0}], ids=["new-1"])
    st.similarity_search("doc 1", k=3, expr='source == "a.pdf"')
    assert st._field_map_builds == 3
    assert np.array_equal(st._index.calls[-1], _rows_where(st, a_pdf)) and st._pk_to_row["new-1"] in st._index.calls[-1]
    # upsert: the old row of the pk leaves the map
    old = st._pk_to_row["pk000"]
    st.add_texts(["doc 0 again"], [{"source": "a.pdf", "lang": "en", "page": 0}], ids=["pk000"])
    st.similarity_search("doc 1", k=3, expr='source == "a.pdf"')
    assert st._field_map_builds == 4 and old not in st._index.calls[-1] and st._pk_to_row["pk000"] in st._index.calls[-1]
    # delete
    st.delete(expr='lang == "nl"')
    st.similarity_search("doc 1", k=3, expr='source == "a.pdf"')
    rows = st._index.calls[-1]
    assert np.array_equal(rows, _rows_where(st, a_pdf)) and all(st._metas[r]["lang"] == "en" for r in rows)
    builds = st._field_map_builds
    # compact: the rows are renumbered
    assert st.compact() > 0
    got = st.similarity_search("doc 1", k=200, expr='source == "a.pdf"')
    assert st._field_map_builds == builds + 1
    rows = st._index.calls[-1]
    assert np.array_equal(rows, _rows_where(st, a_pdf)) and rows.max() < len(st._index)
    assert len(got) == rows.size and all(d.metadata["source"] == "a.pdf" for d in got)
    st.similarity_search("doc 3", k=3, expr='source == "a.pdf"')
    assert st._field_map_builds == builds + 1


FILTERS = [
    (dict(expr='source == "a.pdf"'), lambda m, pk: m["source"] == "a.pdf"),
    (dict(filter={"source": "b.pdf", "lang": "nl"}), lambda m, pk: m["source"] == "b.pdf" and m["lang"] == "nl"),
    (dict(expr="source in ['a.pdf', \"c.pdf\"] && lang == 'en'"), lambda m, pk: m["source"] in ("a.pdf", "c.pdf") and m["lang"] == "en"),
    (dict(filter={"page": [1, 2]}, expr='lang == "en"'), lambda m, pk: m["page"] in (1, 2) and m["lang"] == "en"),
    (dict(filter={"pk": ["pk003", "pk010", "pk200"]}), lambda m, pk: pk in ("pk003", "pk010", "pk200")),
]


def _entry_points(st, query, kw):
    """every search entry point -> (name, list of Documents)"""
    vec = HashEmbeddings().embed_query(query)
    yield "similarity_search", st.similarity_search(query, k=5, **kw)
    yield "with_score", [d for d, _ in st.similarity_search_with_score(query, k=5, **kw)]
    yield "with_score_by_vector", [d for d, _ in st.similarity_search_with_score_by_vector(vec, k=5, **kw)]
    yield "with_relevance_scores", [d for d, _ in st.similarity_search_with_relevance_scores(query, k=5, **kw)]
    yield "with_score_batch", [d for d, _ in st.similarity_search_with_score_batch([query, "doc 9"], k=5, **kw)[0]]
    yield "mmr", st.max_marginal_relevance_search(query, k=3, fetch_k=12, **kw)
    yield "mmr_by_vector", st.max_marginal_relevance_search_by_vector(vec, k=3, fetch_k=12, **kw)
    yield "mmr_batch", st.max_marginal_relevance_search_batch([query, "doc 9"], k=3, fetch_k=12, **kw)[0]
    yield "retriever", st.as_retriever(search_kwargs={"k": 5, **kw}).invoke(query)
    yield "retriever_mmr", st.as_retriever(search_type="mmr", search_kwargs={"k": 3, "fetch_k": 12, **kw}).invoke(query)
    yield "retriever_threshold", st.as_retriever(search_type="similarity_score_threshold",
                                                 search_kwargs={"k": 5, "score_threshold": -10.0, **kw}).invoke(query)
    yield "retriever_batch", st.as_retriever(search_kwargs={"k": 5, **kw}).batch_invoke([query, "doc 9"])[0]
    yield "retriever_mmr_batch", st.as_retriever(search_type="mmr", search_kwargs={"k": 3, "fetch_k": 12, **kw}).batch_invoke([query, "doc 9"])[0]


@pytest.mark.parametrize("which", range(len(FILTERS)))
def test_every_entry_point_hands_the_resolved_rows_to_the_index(which):
    kw, keep = FILTERS[which]
    full, part = _store(), _store(keep)
    want_rows = _rows_where(full, keep)
    assert want_rows.size > 0
    for query in ("doc 7", "doc 100", "something else"):
        plain = dict(_entry_points(part, query, {}))
        for name, docs in _entry_points(full, query, kw):
            rows = full._index.calls[-1]
            assert rows is not None and np.array_equal(rows, want_rows), name
            assert docs and all(keep(d.metadata, d.metadata["pk"]) for d in docs), name
            # ... and the answer is that of a store holding only the matching records
            assert [d.page_content for d in docs] == [d.page_content for d in plain[name]], name
    # unfiltered calls still reach the index without `rows`
    full._index.calls.clear()
    for name, docs in _entry_points(full, "doc 7", {}):
        assert docs, name
    assert full._index.calls and all(c is None for c in full._index.calls)


def test_a_filter_that_matches_nothing_returns_an_empty_list():
    st = _store()
    st._index.calls.clear()
    for kw in (dict(expr='source == "nowhere.pdf"'), dict(filter={"lang": "fr"}), dict(filter={"source": "a.pdf"}, expr='source == "b.pdf"'),
               dict(filter={"no_such_field": "x"})):
        for name, docs in _entry_points(st, "doc 7", kw):
            assert docs == [], (name, kw)
    assert st._index.calls == []                         # nothing to search
    with pytest.raises(ValueError):
        st.similarity_search("doc 7", k=3, expr='source ~ "a"')
    with pytest.raises(ValueError):
        st.as_retriever(search_kwargs={"k": 3, "expr": "page > 2"}).invoke("doc 7")


def test_an_index_without_rows_keeps_working_for_unfiltered_calls():
    """The store passes rows= only when a filter was given: an index whose search is (q, k, row_base=0) is never handed the argument."""
    class OldIndex(NumpyIndex):
        def search(self, q, k, row_base=0):
            return NumpyIndex.search(self, q, k, row_base)

    class OldStore(NumpyStore):
        def _new_index(self, dim):
            return OldIndex(dim)

    st = _store(cls=OldStore)
    assert len(st.similarity_search("doc 7", k=4)) == 4
    assert len(st.max_marginal_relevance_search("doc 7", k=3)) == 3
    assert st.delete(expr='source == "a.pdf"').delete_count == 80
    assert st.delete(filter={"source": ["b.pdf", "zzz"], "lang": "nl"}).delete_count == 40
    assert len(st) == 120


# ---- the new kernels' resources -------------------------------------------------------------------------------------------------
def test_the_subset_kernels_use_no_scratch(tmp_path, librmu):
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
            if "scan_subset_kernel" in name or "k_subset_" in name:
                seen[name] = int(scratch)
    scans = [n for n in seen if "scan_subset_kernel" in n]
    assert len(scans) == 9, sorted(seen)                 # three widths x (32 queries, 128 queries, 128 queries with deep slots)
    assert any("k_subset_narrow" in n for n in seen) and any("k_subset_map" in n for n in seen)
    assert all(v == 0 for v in seen.values()), {n[:80]: v for n, v in seen.items() if v}
