"""CPU: the host half of the BM25 index (include/rmu.h, "BM25 retriever") -- argument checks, the whitespace tokenizer and the corpus
statistics against a collections.Counter restatement over str.split(), the binding, the retriever's preprocess_func validation.
Adding documents never touches the GPU, so all of this runs on the GPU-less builder."""
import ctypes
from collections import Counter

import numpy as np
import pytest

from tests.bm25_ref import WHITESPACE, BM25Ref, synth_corpus

NAMES = ["rmu_bm25_create", "rmu_bm25_free", "rmu_bm25_add_texts", "rmu_bm25_stat", "rmu_bm25_df", "rmu_bm25_set_option", "rmu_bm25_search"]


def test_binding_lists_the_bm25_symbols(librmu):
    from ragmeup_amd import _native
    for n in NAMES:
        assert n in _native.SYMBOLS and hasattr(librmu, n), n
    import ragmeup_amd
    assert ragmeup_amd.BM25Index and ragmeup_amd.MI355XBM25Retriever


def test_bad_arguments_fail_before_any_hip_call(librmu):
    h = ctypes.c_void_p()
    d = ctypes.c_double()
    n = ctypes.c_int64()
    assert librmu.rmu_bm25_create(None, 1.5, 0.75, 0.25) == -1
    for k1, b, eps in ((-1.0, 0.75, 0.25), (float("nan"), 0.75, 0.25), (1.5, 1.5, 0.25), (1.5, -0.1, 0.25), (1.5, 0.75, float("inf"))):
        assert librmu.rmu_bm25_create(ctypes.byref(h), k1, b, eps) == -1
        assert b"rmu_bm25_create" in librmu.rmu_last_error()
    assert librmu.rmu_bm25_create(ctypes.byref(h), 1.5, 0.75, 0.25) == 0
    try:
        assert librmu.rmu_bm25_add_texts(None, b"a\0", 2, 1, None) == -1
        assert librmu.rmu_bm25_add_texts(h, None, 2, 1, None) == -1
        assert librmu.rmu_bm25_add_texts(h, b"a\0", 2, -1, None) == -1
        assert librmu.rmu_bm25_add_texts(h, b"a\0b", 3, 2, None) == -1          # the last string is not terminated
        assert librmu.rmu_bm25_add_texts(h, b"a\0b\0", 4, 1, None) == -1        # more strings than n
        assert librmu.rmu_bm25_add_texts(h, b"a\0", 2, 2, None) == -1           # fewer
        assert b"NUL-terminated" in librmu.rmu_last_error()
        assert librmu.rmu_bm25_stat(h, 1, ctypes.byref(d)) == 0 and d.value == 0           # nothing was added by the failed calls
        assert librmu.rmu_bm25_stat(h, 99, ctypes.byref(d)) == -1
        assert librmu.rmu_bm25_stat(h, 1, None) == -1 and librmu.rmu_bm25_stat(None, 1, ctypes.byref(d)) == -1
        assert librmu.rmu_bm25_df(h, None, ctypes.byref(n)) == -1 and librmu.rmu_bm25_df(h, b"a", None) == -1
        for opt, val in ((1, 63), (1, 96), (1, 16384), (1, -64), (2, -1), (2, 1025), (3, 1)):
            assert librmu.rmu_bm25_set_option(h, opt, val) == -1, (opt, val)
        assert librmu.rmu_bm25_set_option(None, 1, 64) == -1
        for opt, val in ((1, 64), (1, 8192), (1, 0), (2, 1), (2, 1024), (2, 0)):
            assert librmu.rmu_bm25_set_option(h, opt, val) == 0, (opt, val)
        s = np.zeros(4, np.float32)
        r = np.zeros(4, np.int64)
        sp, rp = s.ctypes.data, r.ctypes.data
        assert librmu.rmu_bm25_search(None, b"a\0", 2, 1, 4, 0, sp, rp, 0) == -1
        assert librmu.rmu_bm25_search(h, None, 2, 1, 4, 0, sp, rp, 0) == -1
        assert librmu.rmu_bm25_search(h, b"a\0", 2, 1, 4, 0, None, rp, 0) == -1
        assert librmu.rmu_bm25_search(h, b"a\0", 2, 1, 4, 0, sp, None, 0) == -1
        assert librmu.rmu_bm25_search(h, b"a\0", 2, 0, 4, 0, sp, rp, 0) == -1
        assert librmu.rmu_bm25_search(h, b"a\0", 2, 1, 0, 0, sp, rp, 0) == -1
        assert librmu.rmu_bm25_search(h, b"a\0", 2, 1, 113, 0, sp, rp, 0) == -1
        assert b"RMU_MAX_K" in librmu.rmu_last_error()
        assert librmu.rmu_bm25_search(h, b"a", 1, 1, 4, 0, sp, rp, 0) == -1
        long_q = (" ".join(["t"] * 1025) + "\0").encode()
        assert librmu.rmu_bm25_search(h, long_q, len(long_q), 1, 4, 0, sp, rp, 0) == -1
        assert b"1024 tokens" in librmu.rmu_last_error()
        # an empty index answers without the device: every slot is (-inf, -1)
        assert librmu.rmu_bm25_search(h, b"a\0", 2, 1, 4, 0, sp, rp, 0) == 0
        assert np.all(np.isneginf(s)) and np.all(r == -1)
    finally:
        assert librmu.rmu_bm25_free(h) == 0
    assert librmu.rmu_bm25_free(None) == 0


def _tricky_corpus():
    """Every whitespace code point between two tokens, multi-byte tokens, empty and whitespace-only documents, non-whitespace look-alikes."""
    docs = ["", "   ", "plain words plain", "Case case CASE", "café naïve 中文 日本語 😀 café"]
    docs += [f"l{i}{ws}r{ws}{ws}l{i}" for i, ws in enumerate(WHITESPACE)]
    docs += ["".join(WHITESPACE), "x" + "".join(WHITESPACE) + "y"]
    docs += ["zero\u200bwidth a\u180eb no\u2060break \ufeffbom", "tab\there", "punct, punct . ,", "\x1b[0m \x7f"]
    docs += synth_corpus(40, seed=3)
    return docs


def _counter_stats(texts):
    df, nnz, total = Counter(), 0, 0
    for t in texts:
        toks = t.split()
        total += len(toks)
        c = Counter(toks)
        nnz += len(c)
        df.update(c.keys())
    return df, nnz, total


def test_df_and_stat_equal_a_counter_over_str_split(librmu):
    from ragmeup_amd.bm25 import BM25Index
    texts = _tricky_corpus()
    ix = BM25Index()
    try:
        # repeated adds: one by one, a block, an empty add, the rest
        assert ix.add_texts(texts[:1]) == 0
        assert ix.add_texts(texts[1:9]) == 1
        assert ix.add_texts([]) == 9
        assert ix.add_texts(texts[9:]) == 9
        df, nnz, total = _counter_stats(texts)
        st = ix.stat()
        assert st == {"docs": len(texts), "vocab": len(df), "nnz": nnz, "avgdl": total / len(texts)}
        assert len(ix) == len(texts)
        for term, n in df.items():
            assert ix.df(term) == n, ascii(term)
        for absent in ("absent", "Plain", "caf", "l0", "中"):
            assert ix.df(absent) == df.get(absent, 0)
        assert ix.df("r") == len(WHITESPACE)
        ref = BM25Ref(texts)
        assert ref.df == dict(df) and ref.nnz == nnz
        # the same documents again: every df doubles
        ix.add_texts(texts)
        assert ix.stat() == {"docs": 2 * len(texts), "vocab": len(df), "nnz": 2 * nnz, "avgdl": total / len(texts)}
        assert ix.df("café") == 2 * df["café"]
    finally:
        ix.close()


def test_texts_with_nul_are_refused():
    from ragmeup_amd.bm25 import BM25Index
    ix = BM25Index()
    try:
        with pytest.raises(ValueError):
            ix.add_texts(["a\0b"])
        assert len(ix) == 0
    finally:
        ix.close()


def test_retriever_surface_and_preprocess_func_validation(librmu):
    from ragmeup_amd._lc import BaseRetriever, Document
    from ragmeup_amd.bm25 import MI355XBM25Retriever
    r = MI355XBM25Retriever.from_texts(["Alpha beta", "gamma"], metadatas=[{"s": 1}, {"s": 2}], preprocess_func=lambda t: t.lower().split())
    assert isinstance(r, BaseRetriever) and r.k == 4
    assert [d.page_content for d in r.docs] == ["Alpha beta", "gamma"] and r.docs[1].metadata == {"s": 2}
    assert r.vectorizer.df("alpha") == 1 and r.vectorizer.df("Alpha") == 0            # the caller's tokens, not str.split()'s
    r.add_documents([Document(page_content="Delta ALPHA", metadata={"s": 3})])
    assert len(r.docs) == 3 and r.vectorizer.df("alpha") == 2 and r.vectorizer.stat()["docs"] == 3
    for bad in (lambda t: ["ok", ""], lambda t: ["two words"], lambda t: ["tab\tin"], lambda t: ["nbsp\xa0in"], lambda t: [b"bytes"]):
        with pytest.raises(ValueError):
            MI355XBM25Retriever.from_texts(["some text"], preprocess_func=bad)
    r2 = MI355XBM25Retriever.from_documents([Document(page_content="x y", metadata={"a": 1})], bm25_params={"k1": 1.2, "b": 0.5}, k=2)
    assert r2.k == 2 and r2.docs[0].metadata == {"a": 1} and r2.preprocess_func is None
    with pytest.raises(Exception):
        MI355XBM25Retriever.from_texts(["x"], bm25_params={"b": 2.0})
    assert MI355XBM25Retriever.from_texts([]).batch_invoke(["q"]) == [[]]


def test_the_bm25_kernel_has_no_scratch_segment(tmp_path, librmu):
    """both instantiations of bm25_topk_kernel (k <= 64, k <= 112) are in the product library and neither has a private segment"""
    import os
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
    found = {}
    for co in sorted(tmp_path.glob("librmu.so.*gfx950")):
        notes = subprocess.run([readelf, "--notes", str(co)], capture_output=True, text=True).stdout
        for name, scratch in re.findall(r"\.name:\s+(\S+)\n\s+\.private_segment_fixed_size:\s+(\d+)", notes):
            if "bm25_topk_kernel" in name:
                found[name] = int(scratch)
    assert len(found) == 2 and set(found.values()) == {0}, found
