"""CPU: the host reference of the grouped search (tests/distinct_ref.py) on a hand-written case, every argument check of
rmu_index_search_distinct that needs no GPU, the store's routing of group_by= over a stand-in index, and the resources of the new kernels
(the code objects' metadata notes).  The kernels themselves: tests/test_distinct_gpu.py."""
import ctypes
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import distinct_ref as R
from tests import exact_regimes as E
from tests.test_subset_cpu import HashEmbeddings, NumpyIndex, NumpyStore
from tests.test_where_cpu import HostColumns

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _err(librmu):
    return librmu.rmu_last_error().decode()


# ---- the reference, on twelve rows whose answer is written out here ---------------------------------------------------------------------
#        row:   0     1     2     3      4     5     6     7     8     9       10    11
SCORES = [[0.9, 0.9, 0.8, 0.95, 0.7, 0.7, 0.7, 0.5, 0.4, np.nan, 0.3, 0.2]]
CODES = [0, 1, 0, 2, 1, 3, 3, 2, 4, 5, 0, 4]
ALIVE = [1, 1, 1, 0, 1, 1, 1, 1, 1, 1, 1, 1]
# row 3, the best row of all and of group 2, is dead: row 7 represents group 2.  Rows 0 and 1 tie in different groups: row 0 first.  Rows 5
# and 6 tie inside group 3: row 5 represents it.  Group 5 has one row, tombstoned (NaN): absent.  Five live groups.
ORDER = [0, 1, 5, 7, 8]


def test_the_reference_on_a_hand_written_case():
    sc = np.array(SCORES, np.float32)
    alive = np.array(ALIVE, bool)
    for k in (1, 3, 5):
        s, r = R.distinct_from_scores(sc, alive, CODES, k)
        assert r.tolist() == [ORDER[:k]] and s.dtype == np.float32 and r.dtype == np.int64
        assert np.array_equal(E.bits(s), E.bits(sc[:, ORDER[:k]]))
    s, r = R.distinct_from_scores(sc, alive, CODES, 8)                      # fewer than k groups: padding
    assert r.tolist() == [ORDER + [-1, -1, -1]] and np.isneginf(s[0, 5:]).all() and np.array_equal(E.bits(s[:, :5]), E.bits(sc[:, ORDER]))
    s, r = R.distinct_from_scores(sc, alive, CODES, 3, row_base=1000)       # row_base moves the ids, never the padding
    assert r.tolist() == [[1000, 1001, 1005]]
    assert R.distinct_from_scores(sc, alive, CODES, 8, row_base=7)[1][0, 5:].tolist() == [-1, -1, -1]
    # an L2 index ranks by the scan's score and reports max(|q|^2 - s, 0); its padding is +inf
    qn2 = np.array([1.0], np.float32)
    s, r = R.distinct_from_scores(sc, alive, CODES, 6, qn2=qn2)
    assert r.tolist() == [ORDER + [-1]] and np.isposinf(s[0, 5])
    assert np.array_equal(E.bits(s[0, :5]), E.bits(np.float32(1.0) - sc[0, ORDER]))
    # everything dead: all padding
    s, r = R.distinct_from_scores(sc, np.zeros(12, bool), CODES, 4)
    assert (r == -1).all() and np.isneginf(s).all()
    # one group for every row: one hit
    assert R.distinct_from_scores(sc, alive, [7] * 12, 3)[1].tolist() == [[0, -1, -1]]
    # one row per group: the plain top-k
    s, r = R.distinct_from_scores(sc, alive, list(range(12)), 4)
    es, er = E.expected_topk(sc, alive, 4)
    assert np.array_equal(r, er) and np.array_equal(E.bits(s), E.bits(es))


def test_the_planner_restated():
    p = R.plan(40_000, 32)
    assert (p["wq"], p["RT"], p["parts"]) == (1, 128, 4 * p["s_chunks"]) and p["tiles_per_chunk"] * p["s_chunks"] >= p["tiles_total"]
    p = R.plan(40_000, 33)
    assert (p["wq"], p["RT"], p["parts"]) == (4, 32, p["s_chunks"]) and p["parts"] <= 1024
    assert R.plan(1, 1)["parts"] == 4 and R.plan(1, 300)["parts"] == 1


# ---- C-ABI ----------------------------------------------------------------------------------------------------------------------------
def test_the_symbol_is_exported_bound_and_described(librmu):
    from ragmeup_amd import _native
    assert hasattr(librmu, "rmu_index_search_distinct") and "rmu_index_search_distinct" in _native.SYMBOLS
    assert len(librmu.rmu_index_search_distinct.argtypes) == 11
    header = open(os.path.join(ROOT, "include", "rmu.h")).read()
    m = re.search(r"#define RMU_MAX_K_DISTINCT (\d+)", header)
    assert m and int(m.group(1)) == _native.MAX_K_DISTINCT == R.MAX_K == 32
    assert "group_by_field" in header and "out of step" in header


def test_invalid_arguments_fail_before_the_index_is_looked_at(librmu):
    """An index cannot be created without a GPU, and the contract puts these checks in front of everything that reads it: the handle passed
    here is a block of zeros that is never dereferenced."""
    from ragmeup_amd import Columns
    fake = ctypes.addressof(ctypes.create_string_buffer(4096))
    c = Columns(2)
    q = np.zeros((3, 64), np.float32)
    s = np.zeros((3, 32), np.float32)
    r = np.zeros((3, 32), np.int64)

    def call(idx=fake, col=c._h, field=0, qp=q.ctypes.data, nq=3, k=5, flags=0, sp=s.ctypes.data, rp=r.ctypes.data):
        return librmu.rmu_index_search_distinct(idx, col, field, qp, nq, k, flags, 0, sp, rp, 0), _err(librmu)
    for kw in (dict(idx=None), dict(col=None), dict(qp=None), dict(sp=None), dict(rp=None)):
        rc, msg = call(**kw)
        assert rc == -1 and "rmu_index_search_distinct" in msg and "null" in msg, kw
    for k in (0, 33, -1):
        rc, msg = call(k=k)
        assert rc == -1 and "k must be in [1, 32]" in msg
    for nq in (0, -5):
        rc, msg = call(nq=nq)
        assert rc == -1 and "nq" in msg
    for field in (-1, 2):
        rc, msg = call(field=field)
        assert rc == -1 and "field" in msg and "[0, 2)" in msg
    rc, msg = call(flags=8)                                                  # RMU_F_ROWS_DEVICE means nothing here
    assert rc == -1 and "flags" in msg
    c.close()


def test_flatindex_search_distinct_signature():
    from ragmeup_amd.index import FlatIndex
    sig = inspect.signature(FlatIndex.search_distinct)
    assert list(sig.parameters)[1:] == ["q", "k", "columns", "field", "row_base"] and sig.parameters["row_base"].default == 0


# ---- the store over a CPU stand-in index ------------------------------------------------------------------------------------------------
class DistinctIndex(NumpyIndex):
    """NumpyIndex + search_distinct in numpy over a stand-in for the code rows; records its calls; can be told to refuse some of them the
    way the library does when an insert ran beside the search."""

    def __init__(self, dim):
        super().__init__(dim)
        self.distinct_calls = []
        self.refuse = 0                                     # how many of the next calls meet "out of step"

    def search_distinct(self, q, k, columns, field, row_base=0):
        from ragmeup_amd import _native as N
        q = np.asarray(q, np.float32).reshape(-1, self.dim)
        self.distinct_calls.append((q.shape[0], k, field))
        codes = columns.codes()
        if self.refuse > 0 or codes.shape[0] != len(self):
            self.refuse -= 1
            raise N.RmuError(-1, "rmu_index_search_distinct", f"rmu_index_search_distinct: the columns ({codes.shape[0]} rows) and the "
                                                              f"index ({len(self)} rows) are out of step")
        sc = (q.astype(np.float64) @ self.x.astype(np.float64).T).astype(np.float32)
        return R.distinct_from_scores(sc, self.alive, codes[:, field], k, row_base=row_base)


class DistinctStore(NumpyStore):
    def _new_index(self, dim):
        return DistinctIndex(dim)

    def _new_columns(self, n_fields):
        return HostColumns(n_fields)


def _grouped_store(n=120, fields=("lang", "source"), **kw):
    texts = ["chunk %d" % i for i in range(n)]
    metas = [{"source": "doc%02d.pdf" % (i // 8), "lang": ("en", "nl", "de")[i % 3], "page": i % 8} for i in range(n)]
    st = DistinctStore(embeddings=HashEmbeddings(), collection_name="distinct-cpu", auto_persist=False, device_fields=fields, **kw)
    st.add_texts(texts[:70], metas[:70], ids=["pk%03d" % i for i in range(70)])
    st.add_texts(texts[70:], metas[70:], ids=["pk%03d" % i for i in range(70, n)])
    return st


def _expected_sources(st, query, k):
    """the best chunk of each of the k best sources, by walking the plain ranking of every live record"""
    q = np.asarray(st._embeddings.embed_query(query), np.float32)
    ranked = st.similarity_search_with_score_by_vector(q, k=len(st._index))
    seen, out = set(), []
    for d, _ in ranked:
        if d.metadata["source"] not in seen:
            seen.add(d.metadata["source"])
            out.append(d.page_content)
    return out[:k]


def test_group_by_reaches_search_distinct_with_the_column_number_through_every_entry_point():
    st = _grouped_store()
    idx = st._index
    want = _expected_sources(st, "query 0", 4)
    assert len(want) == 4
    got = st.similarity_search("query 0", k=4, group_by="source")
    assert [d.page_content for d in got] == want and len({d.metadata["source"] for d in got}) == 4
    assert idx.distinct_calls == [(1, 4, 1)]                                 # "source" is device field number 1
    assert [d.page_content for d, _ in st.similarity_search_with_score("query 0", k=4, group_by="source")] == want
    assert [d.page_content for d, _ in st.similarity_search_with_relevance_scores("query 0", k=4, group_by="source")] == want
    qv = st._embeddings.embed_query("query 0")
    assert [d.page_content for d, _ in st.similarity_search_with_score_by_vector(qv, k=4, group_by="source")] == want
    queries = ["query %d" % i for i in range(5)]
    del idx.distinct_calls[:]
    batch = st.similarity_search_with_score_batch(queries, k=3, group_by="source")
    assert idx.distinct_calls == [(5, 3, 1)]                                 # one grouped call for the batch
    assert [[d.page_content for d, _ in row] for row in batch] == [_expected_sources(st, q, 3) for q in queries]
    # the retriever: invoke and batch_invoke
    rt = st.as_retriever(search_kwargs={"k": 4, "group_by": "source"})
    assert [d.page_content for d in rt.invoke("query 0")] == want
    assert [[d.page_content for d in row] for row in rt.batch_invoke(queries)] == [_expected_sources(st, q, 4) for q in queries]
    # the other device field: three languages, k = 5 -> three documents
    del idx.distinct_calls[:]
    got = st.similarity_search("query 1", k=5, group_by="lang")
    assert idx.distinct_calls == [(1, 5, 0)] and sorted(d.metadata["lang"] for d in got) == ["de", "en", "nl"]
    # scores are the ungrouped search's for the same documents
    plain = {d.page_content: s for d, s in st.similarity_search_with_score_by_vector(qv, k=len(idx))}
    for d, s in st.similarity_search_with_score_by_vector(qv, k=4, group_by="source"):
        assert s == plain[d.page_content]
    # a delete: the next best chunk of the source takes over; a whole source removed: it is gone
    first = st.similarity_search("query 0", k=1, group_by="source")[0]
    st.delete(ids=["pk%03d" % int(first.page_content.split()[1])])
    assert [d.page_content for d in st.similarity_search("query 0", k=4, group_by="source")] == _expected_sources(st, "query 0", 4)
    st.delete(expr='source == "%s"' % first.metadata["source"])
    got = st.similarity_search("query 0", k=4, group_by="source")
    assert first.metadata["source"] not in {d.metadata["source"] for d in got}
    assert [d.page_content for d in got] == _expected_sources(st, "query 0", 4)
    st.compact()
    assert [d.page_content for d in st.similarity_search("query 0", k=4, group_by="source")] == _expected_sources(st, "query 0", 4)


def test_group_by_refusals_are_value_errors_with_the_reason():
    st = _grouped_store(fields=("source",))
    with pytest.raises(ValueError, match="device_fields="):
        st.similarity_search("q", k=3, group_by="lang")                     # not a device field
    with pytest.raises(ValueError, match="device_fields="):
        st.similarity_search_with_score_batch(["q"], k=3, group_by="pk")
    for kw in (dict(expr='lang == "en"'), dict(filter={"lang": "en"})):
        for call in (st.similarity_search, st.similarity_search_with_score, st.similarity_search_with_relevance_scores):
            with pytest.raises(ValueError, match="cannot be combined"):
                call("q", k=3, group_by="source", **kw)
        with pytest.raises(ValueError, match="cannot be combined"):
            st.similarity_search_with_score_by_vector(st._embeddings.embed_query("q"), k=3, group_by="source", **kw)
        with pytest.raises(ValueError, match="cannot be combined"):
            st.similarity_search_with_score_batch(["q", "r"], k=3, group_by="source", **kw)
    for kw in (dict(exprs=['lang == "en"', None]), dict(filters=[None, {"lang": "en"}])):
        with pytest.raises(ValueError, match="cannot be combined"):
            st.similarity_search_with_score_batch(["q", "r"], k=3, group_by="source", **kw)
    with pytest.raises(ValueError, match="k <= 32"):
        st.similarity_search("q", k=33, group_by="source")
    qv = st._embeddings.embed_query("q")
    for call, args in ((st.max_marginal_relevance_search, ("q",)), (st.max_marginal_relevance_search_by_vector, (qv,)),
                       (st.max_marginal_relevance_search_batch, (["q"],))):
        with pytest.raises(ValueError, match="MMR"):
            call(*args, k=3, fetch_k=10, group_by="source")
    with pytest.raises(ValueError, match="MMR"):
        st.as_retriever(search_type="mmr", search_kwargs={"k": 3, "group_by": "source"}).invoke("q")
    with pytest.raises(ValueError, match="MMR"):
        st.as_retriever(search_type="mmr", search_kwargs={"k": 3, "group_by": "source"}).batch_invoke(["q"])
    assert st._index.distinct_calls == []                                    # nothing reached the index
    st._index.dim = 1024                                                     # a store wider than 768 dimensions
    with pytest.raises(ValueError, match="768"):
        st.similarity_search("q", k=3, group_by="source")
    st._index.dim = 48
    # a field that received an unhashable value is demoted: no grouped search over it
    st.add_texts(["odd"], [{"source": ["a", "list"]}], ids=["odd"])
    assert "source" in st._dev_demoted
    with pytest.raises(ValueError, match="device_fields="):
        st.similarity_search("q", k=3, group_by="source")


def test_out_of_step_is_retried_a_bounded_number_of_times():
    from ragmeup_amd import _native as N
    st = _grouped_store(fields=("source",))
    idx = st._index
    want = _expected_sources(st, "query 2", 3)
    idx.refuse = 2                                                           # an insert ran beside two attempts
    assert [d.page_content for d in st.similarity_search("query 2", k=3, group_by="source")] == want
    assert len(idx.distinct_calls) == 3
    # the code rows really behind the index: the retry brings them up
    del idx.distinct_calls[:]
    idx.add(np.asarray(st._embeddings.embed_documents(["late"]), np.float32))
    st._texts.append("late"); st._metas.append({"source": "late.pdf"}); st._pks.append("late"); st._alive.append(True)
    assert len(st._columns) == len(idx) - 1
    got = st.similarity_search("late", k=2, group_by="source")
    assert got[0].page_content == "late" and len(st._columns) == len(idx) and len(idx.distinct_calls) == 1
    # never ending refusals end in the library's error, after MAX + 1 attempts
    del idx.distinct_calls[:]
    idx.refuse = 10 ** 6
    with pytest.raises(N.RmuError, match="out of step"):
        st.similarity_search("query 2", k=3, group_by="source")
    assert len(idx.distinct_calls) == st._MAX_OUT_OF_STEP + 1


# ---- the new kernels' resources ---------------------------------------------------------------------------------------------------------
def test_the_distinct_kernels_use_no_scratch(tmp_path, librmu):
    """The way tests/test_subset_cpu.py reads it: the code objects inside librmu.so carry every kernel's resources."""
    from ragmeup_amd import _native
    objdump, readelf = "/opt/rocm/lib/llvm/bin/llvm-objdump", "/opt/rocm/lib/llvm/bin/llvm-readelf"
    if not (os.path.exists(objdump) and os.path.exists(readelf)):
        pytest.skip("ROCm's llvm-objdump / llvm-readelf are not installed")
    so = tmp_path / "librmu.so"
    product = os.path.join(os.path.dirname(_native.__file__), "lib", "librmu.so")
    shutil.copy(product if os.path.exists(product) else _native.SO_PATH, so)
    assert subprocess.run([objdump, "--offloading", str(so)], capture_output=True, text=True, cwd=tmp_path).returncode == 0
    seen = {}
    for co in sorted(tmp_path.glob("librmu.so.*gfx950")):
        notes = subprocess.run([readelf, "--notes", str(co)], capture_output=True, text=True).stdout
        for name, scratch in re.findall(r"\.name:\s+(\S+)\n\s+\.private_segment_fixed_size:\s+(\d+)", notes):
            if "scan_distinct_kernel" in name or "k_distinct_fold" in name:
                seen[name] = int(scratch)
    assert len([n for n in seen if "scan_distinct_kernel" in n]) == 6, sorted(seen)      # three widths x (32 queries, 128 queries)
    assert len([n for n in seen if "k_distinct_fold" in n]) == 1, sorted(seen)
    assert all(v == 0 for v in seen.values()), {n[:80]: v for n, v in seen.items() if v}
