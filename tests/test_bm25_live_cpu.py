"""CPU: removal, compaction and persistence of the BM25 index (include/rmu.h, "Live documents") -- none of rmu_bm25_remove_docs, _stat, _df,
_compact, _save and _load touches the device -- and the retriever's delete / compact / persist / load over it."""
import ctypes
import os
import struct

import numpy as np
import pytest

from tests.bm25_live import OPT_REPACK, LiveCorpus
from tests.test_bm25_cpu import _counter_stats, _tricky_corpus

NAMES = ["rmu_bm25_remove_docs", "rmu_bm25_search_subset", "rmu_bm25_compact", "rmu_bm25_save", "rmu_bm25_load"]
HEADER = 64      # magic 8 | version 4 + 4 | k1, b, epsilon | N, V, nnz


def test_binding_lists_the_new_symbols_and_constants(librmu):
    from ragmeup_amd import _native
    for n in NAMES:
        assert n in _native.SYMBOLS and hasattr(librmu, n), n
    assert _native.BM25_OPT_REPACK_ON_REMOVE == 4 and _native.BM25_STAT_LIVE_DOCS == 5


def _ptr(a):
    return a.ctypes.data


def test_bad_arguments_of_the_new_entry_points(librmu, tmp_path):
    h = ctypes.c_void_p()
    n = ctypes.c_int64(-7)
    d = ctypes.c_double()
    assert librmu.rmu_bm25_create(ctypes.byref(h), 1.5, 0.75, 0.25) == 0
    try:
        assert librmu.rmu_bm25_add_texts(h, b"a b\0b c\0c\0", 10, 3, None) == 0
        ids = np.array([0, 2], np.int64)
        # remove_docs
        assert librmu.rmu_bm25_remove_docs(None, _ptr(ids), 2, ctypes.byref(n)) == -1
        assert librmu.rmu_bm25_remove_docs(h, None, 2, ctypes.byref(n)) == -1
        assert librmu.rmu_bm25_remove_docs(h, _ptr(ids), -1, ctypes.byref(n)) == -1
        for bad in ([0, 3], [-1], [1, 1 << 40]):
            a = np.array(bad, np.int64)
            assert librmu.rmu_bm25_remove_docs(h, _ptr(a), len(a), ctypes.byref(n)) == -1, bad
            assert b"rmu_bm25_remove_docs" in librmu.rmu_last_error()
        assert librmu.rmu_bm25_stat(h, 5, ctypes.byref(d)) == 0 and d.value == 3          # the failed calls changed nothing
        assert librmu.rmu_bm25_remove_docs(h, None, 0, ctypes.byref(n)) == 0 and n.value == 0
        # options: 4 takes 0 or 1, 3 stays unknown
        for opt, val in ((4, 2), (4, -1), (3, 0), (5, 1)):
            assert librmu.rmu_bm25_set_option(h, opt, val) == -1, (opt, val)
        assert librmu.rmu_bm25_set_option(h, 4, 1) == 0 and librmu.rmu_bm25_set_option(h, 4, 0) == 0
        assert librmu.rmu_bm25_stat(h, 6, ctypes.byref(d)) == -1
        # compact
        m = np.zeros(8, np.int64)
        assert librmu.rmu_bm25_compact(None, _ptr(m), 8, ctypes.byref(n)) == -1
        assert librmu.rmu_bm25_compact(h, None, 8, ctypes.byref(n)) == -1
        assert librmu.rmu_bm25_compact(h, _ptr(m), 2, ctypes.byref(n)) == -1
        assert b"rmu_bm25_compact" in librmu.rmu_last_error()
        # search_subset: the list is checked before anything reaches the device
        s, r = np.zeros(4, np.float32), np.zeros(4, np.int64)
        for bad in ([1, 0], [0, 0], [0, 3], [-1, 0]):
            a = np.array(bad, np.int64)
            assert librmu.rmu_bm25_search_subset(h, b"a\0", 2, 1, 4, 0, _ptr(a), len(a), _ptr(s), _ptr(r), 0) == -1, bad
            assert b"ascending" in librmu.rmu_last_error()
        assert librmu.rmu_bm25_search_subset(h, b"a\0", 2, 1, 4, 0, None, 2, _ptr(s), _ptr(r), 0) == -1
        assert librmu.rmu_bm25_search_subset(h, b"a\0", 2, 1, 4, 0, _ptr(ids), -1, _ptr(s), _ptr(r), 0) == -1
        assert librmu.rmu_bm25_search_subset(None, b"a\0", 2, 1, 4, 0, _ptr(ids), 2, _ptr(s), _ptr(r), 0) == -1
        assert librmu.rmu_bm25_search_subset(h, b"a\0", 2, 1, 4, 0, _ptr(ids), 2, None, _ptr(r), 0) == -1
        assert librmu.rmu_bm25_search_subset(h, b"a\0", 2, 1, 113, 0, _ptr(ids), 2, _ptr(s), _ptr(r), 0) == -1
        # an empty list answers without the device
        assert librmu.rmu_bm25_search_subset(h, b"a\0", 2, 1, 4, 0, None, 0, _ptr(s), _ptr(r), 0) == 0
        assert np.all(np.isneginf(s)) and np.all(r == -1)
        # save / load
        path = str(tmp_path / "x.bm25").encode()
        g = ctypes.c_void_p()
        assert librmu.rmu_bm25_save(None, path) == -1 and librmu.rmu_bm25_save(h, None) == -1
        assert librmu.rmu_bm25_save(h, str(tmp_path / "no" / "such" / "dir.bm25").encode()) == -1
        assert librmu.rmu_bm25_load(None, path) == -1 and librmu.rmu_bm25_load(ctypes.byref(g), None) == -1
        assert librmu.rmu_bm25_load(ctypes.byref(g), path) == -1 and b"cannot open" in librmu.rmu_last_error()
    finally:
        assert librmu.rmu_bm25_free(h) == 0


def _expect(corpus: LiveCorpus, docs=None):
    df, nnz, total = _counter_stats(corpus.live_texts)
    n_live = int(corpus.alive.sum())
    st = {"docs": len(corpus.texts) if docs is None else docs, "vocab": len(df), "nnz": nnz, "avgdl": total / n_live if n_live else 0.0}
    if n_live != st["docs"]:
        st["live"] = n_live
    return st, df


def _same_statistics(ix, corpus: LiveCorpus, vocabulary):
    st, df = _expect(corpus)
    assert ix.stat() == st and ix.live == int(corpus.alive.sum())
    for term in vocabulary:
        assert ix.df(term) == df.get(term, 0), ascii(term)


def test_stat_and_df_follow_removals(librmu):
    from ragmeup_amd.bm25 import BM25Index
    texts = _tricky_corpus()
    vocabulary = set(" ".join(texts).split()) | {"absent"}
    c = LiveCorpus(texts)
    ix = BM25Index()
    try:
        ix.add_texts(texts)
        _same_statistics(ix, c, vocabulary)
        assert "live" not in ix.stat()
        # the empty documents, the only holders of some words, a block; an id twice and an id that is already removed count once
        for ids in ([0, 1], [4], [2, 3, 3, 2], list(range(10, 40)), [4, 41, 41]):
            assert ix.remove(ids) == c.remove(ids), ids
            _same_statistics(ix, c, vocabulary)
        assert ix.df("café") == 0 and ix.df("plain") == 0
        assert ix.remove([4]) == 0 and ix.remove([]) == 0
        _same_statistics(ix, c, vocabulary)
        # documents added after a removal continue the ids; a removed word comes back
        assert ix.add_texts(["café again", ""]) == len(texts)
        c.add(["café again", ""])
        _same_statistics(ix, c, vocabulary | {"again"})
        assert ix.df("café") == 1
    finally:
        ix.close()


def test_removing_everything_answers_like_an_empty_index_without_the_device(librmu):
    from ragmeup_amd.bm25 import BM25Index
    texts = _tricky_corpus()
    ix = BM25Index()
    try:
        ix.add_texts(texts)
        assert ix.remove(range(len(texts))) == len(texts)
        assert ix.stat() == {"docs": len(texts), "vocab": 0, "nnz": 0, "avgdl": 0.0, "live": 0}
        assert ix.df("plain") == 0
        for kw in ({}, {"docs": np.arange(5)}):
            s, d = ix.search(["plain words", ""], 7, **kw)
            assert np.all(np.isneginf(s)) and np.all(d == -1)
        m = ix.compact()
        assert np.array_equal(m, np.full(len(texts), -1)) and ix.stat() == {"docs": 0, "vocab": 0, "nnz": 0, "avgdl": 0.0}
        assert ix.add_texts(["plain"]) == 0 and ix.df("plain") == 1
    finally:
        ix.close()


def test_compact_renumbers_and_equals_a_fresh_index(librmu):
    from ragmeup_amd.bm25 import BM25Index
    texts = _tricky_corpus()
    vocabulary = set(" ".join(texts).split())
    c = LiveCorpus(texts)
    ix, fresh = BM25Index(), BM25Index()
    try:
        ix.add_texts(texts)
        # no removed document: the identity, nothing changes
        assert np.array_equal(ix.compact(), np.arange(len(texts)))
        _same_statistics(ix, c, vocabulary)
        ids = [0, 2, 4, 5, 6, 30, len(texts) - 1]
        assert ix.remove(ids) == c.remove(ids)
        want = c.compact()
        m = np.full(len(texts) + 3, 99, np.int64)                   # a longer map: the entries past the documents hold -1
        n = ctypes.c_int64()
        assert librmu.rmu_bm25_compact(ix._h, m.ctypes.data, m.size, ctypes.byref(n)) == 0 and n.value == len(c.texts)
        assert np.array_equal(m[:len(texts)], want) and np.all(m[len(texts):] == -1)
        fresh.add_texts(c.texts)
        assert ix.stat() == fresh.stat() == _expect(c)[0] and len(ix) == len(c.texts)
        for term in vocabulary:
            assert ix.df(term) == fresh.df(term), ascii(term)
        assert np.array_equal(ix.compact(), np.arange(len(c.texts)))
        assert ix.add_texts(["x"]) == len(c.texts)
    finally:
        ix.close()
        fresh.close()


def _saved(tmp_path, name="ix.bm25"):
    """a saved index with removed documents, a term without postings (after a compact) and an added document; + the file's sections"""
    from ragmeup_amd.bm25 import BM25Index
    texts = _tricky_corpus()
    ix = BM25Index(k1=1.2, b=0.6, epsilon=0.3)
    ix.add_texts(texts)
    ix.remove([2, 7])
    ix.compact()
    ix.remove([0, 3, 20])
    ix.add_texts(["plain tail"])
    path = str(tmp_path / name)
    ix.save(path)
    blob = open(path, "rb").read()
    n, v, nnz = struct.unpack_from("<QQQ", blob, 40)
    at = HEADER + 5 * n
    for _ in range(v):
        at += 4 + struct.unpack_from("<I", blob, at)[0]
    bounds = {"magic": 8, "version": 16, "params": 40, "header": HEADER, "dl": HEADER + 4 * n, "live": HEADER + 5 * n, "terms": at,
              "offsets": at + 8 * (v + 1), "docs": at + 8 * (v + 1) + 4 * nnz, "tfs": at + 8 * (v + 1) + 8 * nnz}
    assert bounds["tfs"] == len(blob) and blob[:8] == b"RMUBM25\0"
    return ix, path, blob, bounds, (n, v, nnz)


def test_save_load_round_trip(librmu, tmp_path):
    from ragmeup_amd.bm25 import BM25Index
    ix, path, blob, bounds, (n, v, nnz) = _saved(tmp_path)
    try:
        assert struct.unpack_from("<ddd", blob, 16) == (1.2, 0.6, 0.3)
        live = np.frombuffer(blob, np.uint8, n, bounds["dl"])
        assert n == len(ix) and live.sum() == ix.live and not live[0] and not live[3] and live[1]
        back = BM25Index.load(path)
        try:
            assert back.stat() == ix.stat() and back.live == ix.live
            for term in set(" ".join(_tricky_corpus()).split()) | {"tail", "absent"}:
                assert back.df(term) == ix.df(term), ascii(term)
            # the liveness survives: removing the removed ones again removes nothing, each live one is removed once
            assert back.remove(np.flatnonzero(live == 0)) == 0
            assert back.remove(np.arange(n)) == ix.live
            # and a file written from the loaded index is the same file (tombstones and empty terms included)
            again = BM25Index.load(path)
            try:
                again.save(path + ".2")
                assert open(path + ".2", "rb").read() == blob
            finally:
                again.close()
        finally:
            back.close()
    finally:
        ix.close()


def test_load_refuses_short_long_and_inconsistent_files(librmu, tmp_path):
    from ragmeup_amd.bm25 import BM25Index
    ix, path, blob, bounds, (n, v, nnz) = _saved(tmp_path)
    ix.close()

    def refused(data, what):
        bad = str(tmp_path / "bad.bm25")
        with open(bad, "wb") as f:
            f.write(data)
        h = ctypes.c_void_p()
        assert librmu.rmu_bm25_load(ctypes.byref(h), bad.encode()) == -1, what
        msg = librmu.rmu_last_error()
        assert b"rmu_bm25_load" in msg and b"bad.bm25" in msg, (what, msg)
        assert not h.value

    def patched(at, fmt, *vals):
        b = bytearray(blob)
        struct.pack_into(fmt, b, at, *vals)
        return bytes(b)

    for name, at in bounds.items():
        if name != "tfs":
            refused(blob[:at], f"truncated after {name}")
        refused(blob[:at - 1], f"truncated inside {name}")
    refused(b"", "empty")
    refused(blob + b"\0", "one trailing byte")
    refused(patched(0, "<8s", b"RMUBM26\0"), "magic")
    refused(patched(8, "<I", 2), "version")
    refused(patched(24, "<d", 1.5), "b out of range")
    refused(patched(bounds["offsets"], "<I", n), "a posting id == N")
    refused(patched(bounds["offsets"], "<I", 0xFFFFFFFF), "a posting id far past N")
    for huge in (nnz + 1, 1 << 40, (1 << 64) - 1):
        refused(patched(56, "<Q", huge), f"nnz = {huge}")
    refused(patched(40, "<Q", 1 << 40), "N larger than the file")
    refused(patched(40, "<Q", (1 << 61) + n), "N whose sizes wrap around")
    refused(patched(48, "<Q", (1 << 61) + v), "V whose sizes wrap around")
    refused(patched(48, "<Q", v + 1), "V + 1")
    refused(patched(bounds["docs"], "<I", 0), "a term frequency of 0")
    refused(patched(bounds["docs"], "<I", struct.unpack_from("<I", blob, bounds["docs"])[0] + 1), "dl differs from the tf sum")
    refused(patched(bounds["dl"], "<B", 2), "a liveness byte of 2")
    refused(patched(bounds["terms"], "<Q", 1), "offsets that do not start at 0")
    refused(patched(bounds["live"], "<I", 0), "an empty term")
    # two postings of one term out of order
    off = struct.unpack_from(f"<{v + 1}Q", blob, bounds["terms"])
    t = next(i for i in range(v) if off[i + 1] - off[i] >= 2)
    a, b = struct.unpack_from("<II", blob, bounds["offsets"] + 4 * off[t])
    refused(patched(bounds["offsets"] + 4 * off[t], "<II", b, a), "postings that descend")
    # the untouched file still loads
    BM25Index.load(path).close()


def test_the_masked_kernel_is_in_the_library_without_scratch(tmp_path, librmu):
    """both instantiations of bm25_masked_kernel (k <= 64, k <= 112), found the way test_the_bm25_kernel_has_no_scratch_segment finds the
    plain kernel's; same LDS as the plain kernel (the bitmap is not staged there)"""
    import re
    import shutil
    import subprocess
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
            if "bm25_masked_kernel" in name or "bm25_topk_kernel" in name:
                scratch[name], lds[name] = int(private), int(lds_bytes)
    masked = [n for n in scratch if "bm25_masked_kernel" in n]
    assert len(masked) == 2 and len(scratch) == 4 and set(scratch.values()) == {0}, scratch
    assert len(set(lds.values())) == 1 and 32768 < next(iter(lds.values())) <= 40960, lds      # four workgroups per CU (160 KiB of LDS)


# ---- the retriever -------------------------------------------------------------------------------------------------------------------
def _retriever(**kw):
    from ragmeup_amd.bm25 import MI355XBM25Retriever
    texts = [f"doc{i} common word{i % 3}" for i in range(12)]
    metas = [{"row": i, "source": f"f{i % 4}.pdf", "page": i % 2} for i in range(12)]
    return MI355XBM25Retriever.from_texts(texts, metadatas=metas, ids=[f"id-{i}" for i in range(12)], **kw), texts, metas


def test_retriever_delete_by_ids_expr_and_filter(librmu):
    r, texts, metas = _retriever()
    try:
        res = r.delete(ids=["id-3", "id-5", "id-unknown"])
        assert res == 2 and res.delete_count == 2
        assert r.delete(ids=["id-3"]).delete_count == 0                                        # already gone
        assert r.delete(expr='source == "f1.pdf"').delete_count == 2                           # rows 1, 9 (5 is gone)
        assert r.delete(filter={"source": "f2.pdf", "page": 0}).delete_count == 3              # rows 2, 6, 10
        assert r.delete(expr='source in ["f0.pdf", "f9.pdf"] and page == 0', filter={"row": [0, 4, 11]}).delete_count == 2
        assert r.delete(expr='pk == "id-7"').delete_count == 1
        assert r.delete().delete_count == 0 and r.delete(ids=[]).delete_count == 0
        with pytest.raises(ValueError):
            r.delete(expr="row > 3")
        # docs[i] stays at position i; the index has forgotten the removed ones
        assert [d.page_content for d in r.docs] == texts and [d.metadata for d in r.docs] == metas
        gone = {3, 5, 1, 9, 2, 6, 10, 0, 4, 7}
        assert r.vectorizer.stat()["live"] == 12 - len(gone) and len(r.vectorizer) == 12
        assert r.vectorizer.df("doc3") == 0 and r.vectorizer.df("doc8") == 1 and r.vectorizer.df("common") == 2
        # compact renumbers docs with the index's map
        assert r.compact() == len(gone) and r.compact() == 0
        assert [d.metadata["row"] for d in r.docs] == [8, 11] and len(r.vectorizer) == 2
        assert r.delete(ids=["id-11"]).delete_count == 1 and r.vectorizer.df("doc11") == 0
        r.add_texts(["fresh text"], [{"row": 12}], ids=["id-12"])
        assert [d.metadata["row"] for d in r.docs] == [8, 11, 12] and r.vectorizer.stat()["live"] == 2
    finally:
        r.vectorizer.close()


def test_retriever_compact_threshold(librmu):
    r, texts, _ = _retriever(compact_threshold=0.25)
    try:
        r.delete(ids=["id-0", "id-1", "id-2"])                     # 3 of 12 is not more than a quarter
        assert len(r.docs) == 12 and r.vectorizer.stat()["live"] == 9
        r.delete(ids=["id-3"])                                     # 4 of 12 is
        assert [d.metadata["row"] for d in r.docs] == list(range(4, 12))
        assert r.vectorizer.stat() == {"docs": 8, "vocab": r.vectorizer.stat()["vocab"], "nnz": 24, "avgdl": 3.0}
        r2, _, _ = _retriever()
        try:
            r2.delete(ids=[f"id-{i}" for i in range(11)])
            assert len(r2.docs) == 12                              # no threshold: never by itself
        finally:
            r2.vectorizer.close()
    finally:
        r.vectorizer.close()


def test_retriever_persist_and_load(librmu, tmp_path):
    from datetime import date
    from ragmeup_amd.bm25 import MI355XBM25Retriever
    r, texts, metas = _retriever(k=3)
    try:
        r.add_texts(["Ünï çödé ☃ text", "no id"], [{"when": date(2024, 1, 2), "n": np.int64(7)}, {}], ids=["id-u", None])
        r.delete(expr='source == "f2.pdf"')
        path = str(tmp_path / "sparse")
        r.persist(path)
        assert os.path.exists(path + ".bm25") and os.path.exists(path + ".docs.jsonl")
        back = MI355XBM25Retriever.load(path, k=3)
        try:
            assert back.k == 3 and back.preprocess_func is None
            assert [d.page_content for d in back.docs] == [d.page_content for d in r.docs]
            assert [d.metadata for d in back.docs[:12]] == metas
            assert back.docs[12].metadata == {"when": "2024-01-02", "n": 7} and back.docs[13].metadata == {}
            assert back.vectorizer.stat() == r.vectorizer.stat() and back.vectorizer.stat()["live"] == 11
            assert back.vectorizer.df("☃") == 1 and back.vectorizer.df("doc2") == 0
            # ids and liveness came back: the removed stay removed, the others are found by their ids
            assert back.delete(ids=["id-2", "id-6", "id-10"]).delete_count == 0
            assert back.delete(ids=["id-u", "id-1"]).delete_count == 2 and back.vectorizer.df("☃") == 0
            assert back.compact() == 5 and len(back.docs) == 9
        finally:
            back.vectorizer.close()
        # records and index out of step
        with open(path + ".docs.jsonl", "a", encoding="utf-8") as f:
            f.write('{"text": "x", "metadata": {}, "id": null, "alive": 1}\n')
        with pytest.raises(ValueError):
            MI355XBM25Retriever.load(path)
    finally:
        r.vectorizer.close()


def test_search_kwargs_select_the_candidate_ids(librmu):
    """the id list behind search_kwargs' filter / expr: ascending live ids, cached until the records change"""
    r, _, _ = _retriever(search_kwargs={"filter": {"source": "f1.pdf"}})
    try:
        assert r._candidates().tolist() == [1, 5, 9]
        assert r._candidates() is r._candidates()
        r.delete(ids=["id-5"])
        assert r._candidates().tolist() == [1, 9]
        r.add_texts(["more"], [{"source": "f1.pdf"}])
        assert r._candidates().tolist() == [1, 9, 12]
        r.search_kwargs = {"expr": 'source == "f1.pdf" and page == 1', "filter": {"row": [1, 2, 9]}}
        assert r._candidates().tolist() == [1, 9]
        r.search_kwargs = {}
        assert r._candidates() is None
        r.search_kwargs = {"expr": "row > 3"}
        with pytest.raises(ValueError):
            r.batch_invoke(["common"])
    finally:
        r.vectorizer.close()
