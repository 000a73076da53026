"""CPU: compaction of tombstoned rows (rmu_index_compact) -- argument checks of the C-ABI, and the vector store's bookkeeping around
MI355XVectorStore.compact() / compact_threshold on an oracle-backed fake index (the GPU side: tests/test_compact_gpu.py)."""
import ctypes
import hashlib
import threading

import numpy as np
import pytest

from oracle import oracle as O
from ragmeup_amd.documents import Document
from ragmeup_amd.vectorstore import MI355XVectorStore


def test_compact_invalid_arguments_fail_without_gpu(librmu):
    """Argument validation happens before any device work, so it is testable on the GPU-less builder."""
    librmu.rmu_index_compact.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int64, ctypes.POINTER(ctypes.c_int64)]
    n = ctypes.c_int64(-7)
    m = np.zeros(4, np.int64)
    assert librmu.rmu_index_compact(None, None, 0, ctypes.byref(n)) == -1
    assert b"rmu_index_compact" in librmu.rmu_last_error()
    assert librmu.rmu_index_compact(None, m.ctypes.data, 4, ctypes.byref(n)) == -1
    # a non-null handle is never touched when n_after is null or map_len is negative
    assert librmu.rmu_index_compact(ctypes.c_void_p(16), m.ctypes.data, 4, None) == -1
    assert librmu.rmu_index_compact(ctypes.c_void_p(16), m.ctypes.data, -1, ctypes.byref(n)) == -1
    assert n.value == -7 and (m == 0).all()


def test_binding_constants_match_the_header():
    from ragmeup_amd import _native as N
    import os
    import re
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "rmu.h")).read()
    val = dict(re.findall(r"#define (RMU_\w+) (-?\d+)", src))
    assert int(val["RMU_OPT_COMPACT_INPLACE"]) == N.OPT_COMPACT_INPLACE
    assert int(val["RMU_STAT_COMPACT_COUNT"]) == N.STAT_COMPACT_COUNT
    assert int(val["RMU_STAT_COMPACT_MS"]) == N.STAT_COMPACT_MS


class CompactingIndex:
    """FlatIndex's interface computed by the oracle, compact() included (what rmu_index_compact promises: live rows keep their order)."""

    def __init__(self, dim):
        self.dim, self.x, self.alive = dim, np.zeros((0, dim), np.float32), np.zeros(0, bool)
        self.compactions = 0

    def __len__(self):
        return self.x.shape[0]

    def add(self, v):
        first = self.x.shape[0]
        self.x = np.concatenate([self.x, np.asarray(v, np.float32)])
        self.alive = np.concatenate([self.alive, np.ones(len(v), bool)])
        return first

    def remove_rows(self, rows):
        n = int(self.alive[list(rows)].sum())
        self.alive[list(rows)] = False
        return n

    def get_rows(self, rows):
        return self.x[list(rows)]

    def search(self, q, k, row_base=0):
        s, r = O.flat_search(np.asarray(q, np.float32).reshape(-1, self.dim), self.x, k, alive=self.alive)
        return s.astype(np.float32), r

    def compact(self):
        m = np.full(len(self.alive), -1, np.int64)
        live = np.flatnonzero(self.alive)
        m[live] = np.arange(live.size)
        self.x, self.alive = self.x[live], np.ones(live.size, bool)
        self.compactions += 1
        return m

    def save(self, path):
        with open(path, "wb") as f:
            np.savez(f, x=self.x, alive=self.alive)

    @classmethod
    def load(cls, path):
        z = np.load(path)
        self = cls(z["x"].shape[1])
        self.x, self.alive = z["x"], z["alive"]
        return self


class Store(MI355XVectorStore):
    def _new_index(self, dim):
        return CompactingIndex(dim)

    def _open_index(self, path):
        return CompactingIndex.load(path)

    def _embed_docs_for_index(self, texts):
        return self._embed_docs(texts)


class HashEmbeddings:
    def embed_documents(self, texts):
        out = []
        for t in texts:
            seed = int(hashlib.md5(t.encode()).hexdigest()[:8], 16)
            v = np.random.default_rng(seed).standard_normal(384)
            out.append((v / np.linalg.norm(v)).tolist())
        return out

    def embed_query(self, t):
        return self.embed_documents([t])[0]


def _docs(n, source, version=0):
    return [Document(page_content=f"chunk {i} of {source} v{version}", metadata={"source": source, "i": i}) for i in range(n)]


def _ids(n, source):
    return [hashlib.md5(f"{source}#{i}".encode()).hexdigest() for i in range(n)]


@pytest.fixture()
def make_store(tmp_path):
    MI355XVectorStore._collections.clear()

    def make(name="c", **kw):
        st = Store.from_documents([], HashEmbeddings(), drop_old=True, connection_args={"uri": str(tmp_path / "data.db")},
                                  collection_name=name, auto_persist=False, **kw)
        return st
    yield make
    MI355XVectorStore._collections.clear()


def _pk_results(st, queries, k=8):
    return [[(d.metadata["pk"], d.page_content, s) for d, s in st.similarity_search_with_score(q, k=k)] for q in queries]


def _mmr_pks(st, queries, k=4):
    return [[d.metadata["pk"] for d in st.max_marginal_relevance_search(q, k=k, fetch_k=20)] for q in queries]


QUERIES = [f"chunk {i} of b.pdf v1" for i in range(0, 40, 7)] + ["chunk 3 of a.pdf v0", "something else"]


def test_compact_keeps_every_record_and_result(make_store):
    st = make_store()
    st.add_documents(_docs(60, "a.pdf"), ids=_ids(60, "a.pdf"))
    st.add_documents(_docs(40, "b.pdf"), ids=_ids(40, "b.pdf"))
    st.add_documents(_docs(30, "c.pdf"), ids=_ids(30, "c.pdf"))
    assert st.delete(expr='source == "c.pdf"').delete_count == 30
    st.add_documents(_docs(40, "b.pdf", version=1), ids=_ids(40, "b.pdf"))        # re-upload: upsert tombstones the old rows
    st.delete(ids=_ids(60, "a.pdf")[::5])
    assert len(st._index) == 170 and len(st) == 60 - 12 + 40
    before = _pk_results(st, QUERIES)
    before_mmr = _mmr_pks(st, QUERIES)
    pk_docs = {pk: (st._texts[r], st._metas[r]) for pk, r in st._pk_to_row.items() if st._alive[r]}   # (deleted pks keep a dead row)

    assert st.compact() == 170 - 88
    assert len(st) == 88 and len(st._index) == 88
    assert len(st._texts) == len(st._metas) == len(st._pks) == len(st._alive) == 88 and all(st._alive)
    assert {pk: (st._texts[r], st._metas[r]) for pk, r in st._pk_to_row.items()} == pk_docs
    assert sorted(st._pk_to_row.values()) == list(range(88))
    assert _pk_results(st, QUERIES) == before
    assert _mmr_pks(st, QUERIES) == before_mmr
    assert st.compact() == 0 and st._index.compactions == 1
    # the store keeps working on the new numbering
    st.delete(ids=_ids(40, "b.pdf")[:10])
    st.add_documents(_docs(5, "d.pdf"), ids=_ids(5, "d.pdf"))
    assert len(st) == 83 and st._pk_to_row[_ids(5, "d.pdf")[0]] == 88
    assert [d.page_content for d in st.similarity_search("chunk 2 of d.pdf v0", k=1)] == ["chunk 2 of d.pdf v0"]


def test_compact_threshold_bounds_a_reupload_loop(make_store):
    ids, n = _ids(500, "a.pdf"), 500
    st = make_store("t", compact_threshold=0.5)
    plain = make_store("p")
    for rnd in range(40):
        docs = _docs(n, "a.pdf", version=rnd)
        st.add_documents(docs, ids=ids)
        plain.add_documents(docs, ids=ids)
        assert len(st._index) <= 2 * n + n
        assert len(st) == len(plain) == n
    assert len(plain._index) == 40 * n                                                   # None: today's behaviour, nothing reclaimed
    assert st._index.compactions >= 19
    assert _pk_results(st, QUERIES[:3] + ["chunk 17 of a.pdf v39"]) == _pk_results(plain, QUERIES[:3] + ["chunk 17 of a.pdf v39"])
    # delete() checks the threshold too
    st.delete(ids=ids[:400])
    assert len(st._index) == 100 and len(st) == 100


def test_compact_threshold_none_and_invalid(make_store):
    with pytest.raises(ValueError):
        make_store("bad", compact_threshold=1.5)
    st = make_store()
    assert st.compact_threshold is None and st.compact() == 0                      # no index yet: nothing to do


def test_persist_load_after_compaction(make_store, tmp_path):
    st = make_store()
    st.add_documents(_docs(50, "a.pdf"), ids=_ids(50, "a.pdf"))
    st.add_documents(_docs(20, "b.pdf"), ids=_ids(20, "b.pdf"))
    st.delete(expr='source == "a.pdf"')
    st.add_documents(_docs(20, "b.pdf", 1), ids=_ids(20, "b.pdf"))
    assert st.compact() == 70
    want = _pk_results(st, QUERIES)
    assert st.persist()
    MI355XVectorStore._collections.clear()
    back = Store.from_documents([], HashEmbeddings(), drop_old=False, connection_args={"uri": str(tmp_path / "data.db")},
                                collection_name="c", auto_persist=False)
    assert len(back._index) == 20 and len(back) == 20
    assert _pk_results(back, QUERIES) == want


def test_a_read_that_overlaps_a_compaction_is_repeated(make_store):
    """The seqlock: a compaction that renumbers the rows between a search and the row -> Document step must not turn a row id into
    another record's Document; the read is repeated on the new numbering."""
    st = make_store()
    st.add_documents(_docs(80, "a.pdf"), ids=_ids(80, "a.pdf"))
    st.delete(ids=_ids(80, "a.pdf")[:40:2])
    q = "chunk 61 of a.pdf v0"
    want = _pk_results(st, [q])
    idx = st._index
    plain_search, fired = idx.search, []

    def racing_search(qq, k, row_base=0):
        out = plain_search(qq, k)                  # row ids of the numbering before the compaction
        if not fired:
            fired.append(1)
            t = threading.Thread(target=st.compact)   # another thread compacts between the search and the records
            t.start()
            t.join()
        return out
    idx.search = racing_search
    got = _pk_results(st, [q])
    assert fired and idx.compactions == 1
    assert got == want
    assert got[0][0][1] == q
