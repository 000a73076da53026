"""CPU: the fusion reference of tests/rrf_ref.py against the oracle and against ragmeup_amd.ensemble; every refusal of rmu_rrf_fuse and of
the rmu_hybrid_* calls that is decided before any HIP call; the numbering of page_content classes."""
import ctypes

import numpy as np
import pytest

from tests.rrf_ref import fuse, fuse_arrays, random_case


def test_the_reference_agrees_with_the_oracle_and_with_the_ensemble_module():
    from oracle import oracle as O
    from ragmeup_amd._lc import Document
    from ragmeup_amd.ensemble import weighted_reciprocal_rank
    rng = np.random.default_rng(11)
    ties = 0
    for case in range(300):
        lists, depth = int(rng.integers(1, 5)), int(rng.integers(1, 113 if case % 10 == 0 else 24))
        keys = random_case(rng, lists, 2, depth)
        w = [[1.0 / lists] * lists, rng.uniform(0, 1, lists).tolist(), [1.0] + [0.0] * (lists - 1)][case % 3]
        c = (60, 0, 1)[case % 3]
        for q in range(2):
            raw = [keys[l, q].tolist() for l in range(lists)]
            kk, ss, src = fuse(raw, w, c)                      # (asserts its order against oracle.weighted_rrf itself)
            compact = [[k for k in lst if k >= 0] for lst in raw]
            assert kk == O.weighted_rrf(compact, w, c)
            docs = [[Document(page_content=f"text {k}", metadata={"list": l, "at": i}) for i, k in enumerate(lst)] for l, lst in enumerate(compact)]
            fused = weighted_reciprocal_rank(docs, w, c)
            assert [d.page_content for d in fused] == [f"text {k}" for k in kk]
            # the representative is the first occurrence in the chain: (list, position among the present entries)
            for d, (l, pos) in zip(fused, src):
                assert d.metadata == {"list": l, "at": sum(1 for k in raw[l][:pos] if k >= 0)}
            assert all(raw[l][pos] == k for k, (l, pos) in zip(kk, src))
            assert all(a >= b for a, b in zip(ss, ss[1:]))
            ties += sum(1 for a, b in zip(ss, ss[1:]) if a == b)
    assert ties > 100
    s, k, r = fuse_arrays(np.array([[[3, 3, -1, 5]], [[5, 9, 3, -1]]], np.int64), [0.5, 0.5], 60, 8)
    assert k[0].tolist() == [3, 5, 9, -1, -1, -1, -1, -1] and r[0].tolist() == [0, 3, 5, -1, -1, -1, -1, -1]
    assert s[0, 0] == 0.0 + 0.5 / 61 + 0.5 / 62 + 0.5 / 63 and np.all(np.isneginf(s[0, 3:]))


def _fuse_rc(lib, keys=True, lists=2, nq=1, depth=4, weights=(0.5, 0.5, 0.5, 0.5, 0.5), c=60, k_out=4, outs=(True, True, True)):
    k = np.zeros((max(lists, 1), max(nq, 1), max(depth, 1)), np.int64)
    w = (ctypes.c_double * len(weights))(*weights) if weights is not None else None
    n = max(1, nq) * max(1, k_out)
    s, o, r = np.empty(n, np.float64), np.empty(n, np.int64), np.empty(n, np.int32)
    return lib.rmu_rrf_fuse(k.ctypes.data if keys else None, lists, nq, depth, w, c, k_out, 0, s.ctypes.data if outs[0] else None,
                            o.ctypes.data if outs[1] else None, r.ctypes.data if outs[2] else None, 0)


def test_rrf_fuse_refuses_bad_arguments_without_a_gpu(librmu):
    lib = librmu
    assert _fuse_rc(lib, lists=0) == -1 and _fuse_rc(lib, lists=5) == -1
    assert b"lists" in lib.rmu_last_error()
    assert _fuse_rc(lib, depth=0, k_out=1) == -1 and _fuse_rc(lib, depth=113) == -1
    assert b"depth" in lib.rmu_last_error()
    assert _fuse_rc(lib, k_out=0) == -1 and _fuse_rc(lib, lists=2, depth=4, k_out=9) == -1
    assert b"k_out" in lib.rmu_last_error()
    assert _fuse_rc(lib, nq=0) == -1
    assert _fuse_rc(lib, weights=(0.5, float("nan"))) == -1 and _fuse_rc(lib, weights=(0.5, -0.25)) == -1
    assert _fuse_rc(lib, weights=(float("inf"), 0.5)) == -1
    assert b"weight" in lib.rmu_last_error()
    assert _fuse_rc(lib, c=-1) == -1
    assert b"c must" in lib.rmu_last_error()
    assert _fuse_rc(lib, keys=False) == -1 and _fuse_rc(lib, weights=None) == -1
    for i in range(3):
        assert _fuse_rc(lib, outs=tuple(j != i for j in range(3))) == -1
    assert b"null" in lib.rmu_last_error()


def _bm25(lib, texts):
    h = ctypes.c_void_p()
    assert lib.rmu_bm25_create(ctypes.byref(h), 1.5, 0.75, 0.25) == 0
    blob = ("\0".join(texts) + "\0").encode()
    assert lib.rmu_bm25_add_texts(h, blob, len(blob), len(texts), None) == 0
    return h


def test_hybrid_create_and_set_keys_refusals_are_host_only(librmu):
    lib = librmu
    h = ctypes.c_void_p()
    sparse = _bm25(lib, ["a b", "b c", "a b"])
    try:
        assert lib.rmu_hybrid_create(None, sparse, None) == -1
        assert lib.rmu_hybrid_create(ctypes.byref(h), None, None) == -1
        assert lib.rmu_hybrid_create(ctypes.byref(h), sparse, None) == 0
        keys = np.array([0, 1, 0], np.int64)
        assert lib.rmu_hybrid_set_keys(h, 0, 1, keys.ctypes.data, 3) == -1             # first beyond the (empty) table
        assert b"beyond" in lib.rmu_last_error()
        assert lib.rmu_hybrid_set_keys(h, 0, 0, keys.ctypes.data, 3) == 0
        assert lib.rmu_hybrid_set_keys(h, 0, 4, keys.ctypes.data, 1) == -1
        assert lib.rmu_hybrid_set_keys(h, 0, 3, keys.ctypes.data, 2) == 0              # an append: 5 keys now
        assert lib.rmu_hybrid_set_keys(h, 0, 6, keys.ctypes.data, 1) == -1 and lib.rmu_hybrid_set_keys(h, 0, 5, keys.ctypes.data, 0) == 0
        bad = np.array([2, -1], np.int64)
        assert lib.rmu_hybrid_set_keys(h, 0, 0, bad.ctypes.data, 2) == -1
        assert b"negative" in lib.rmu_last_error()
        assert lib.rmu_hybrid_set_keys(h, 0, 6, keys.ctypes.data, 1) == -1             # (the refused call changed nothing: still 5 keys)
        assert lib.rmu_hybrid_set_keys(h, 2, 0, keys.ctypes.data, 1) == -1 and lib.rmu_hybrid_set_keys(h, -1, 0, keys.ctypes.data, 1) == -1
        assert lib.rmu_hybrid_set_keys(h, 1, 0, None, 2) == -1 and lib.rmu_hybrid_set_keys(h, 1, 0, keys.ctypes.data, -1) == -1
        assert lib.rmu_hybrid_set_keys(None, 0, 0, keys.ctypes.data, 1) == -1
        assert lib.rmu_hybrid_free(h) == 0 and lib.rmu_hybrid_free(None) == 0
    finally:
        lib.rmu_bm25_free(sparse)


def test_hybrid_search_refuses_bad_arguments_without_a_gpu(librmu):
    lib = librmu
    h = ctypes.c_void_p()
    sparse = _bm25(lib, ["a b", "b c", "a b"])
    assert lib.rmu_hybrid_create(ctypes.byref(h), sparse, None) == 0
    q = np.zeros((2, 8), np.float32)
    w = (ctypes.c_double * 2)(0.5, 0.5)
    s, o, m = np.empty(64, np.float64), np.empty(64, np.int64), np.empty(64, np.int32)
    blob = b"a\0b c\0"

    def rc(hh=h, qq=q.ctypes.data, nq=2, bl=blob, nbytes=None, ks=4, fk=20, kd=4, lam=0.5, ww=w, c=60, k_out=8, outs=(s, o, m)):
        return lib.rmu_hybrid_search(hh, qq, nq, bl, len(bl) if nbytes is None and bl is not None else (nbytes or 0), ks, fk, kd, lam, ww, c, k_out,
                                     *(a.ctypes.data if a is not None else None for a in outs), 0)
    try:
        assert rc(hh=None) == -1 and rc(qq=None) == -1 and rc(bl=None) == -1 and rc(ww=None) == -1
        assert rc(outs=(None, o, m)) == -1 and rc(outs=(s, None, m)) == -1 and rc(outs=(s, o, None)) == -1
        assert b"null" in lib.rmu_last_error()
        assert rc(nq=0) == -1 and rc(nq=65536) == -1
        assert rc(ks=0) == -1 and rc(ks=113) == -1
        assert b"k_sparse" in lib.rmu_last_error()
        assert rc(fk=0) == -1 and rc(fk=65) == -1 and rc(kd=0) == -1 and rc(fk=8, kd=9) == -1
        assert b"fetch_k" in lib.rmu_last_error()
        assert rc(k_out=0) == -1 and rc(k_out=9) == -1
        assert b"k_out" in lib.rmu_last_error()
        assert rc(c=-1) == -1
        assert rc(ww=(ctypes.c_double * 2)(0.5, float("nan"))) == -1 and rc(ww=(ctypes.c_double * 2)(-1.0, 0.5)) == -1
        assert b"weight" in lib.rmu_last_error()
        assert rc(lam=float("nan")) == -1
        assert rc(nq=3) == -1 and rc(bl=b"a\0b c") == -1 and rc(bl=b"a\0b\0c\0") == -1
        assert b"NUL-terminated" in lib.rmu_last_error()
        # the tables against the members: checked before anything is enqueued, so without a GPU too
        assert rc() == -1
        assert b"out of step" in lib.rmu_last_error() and b"sparse" in lib.rmu_last_error()
        keys = np.array([0, 1, 0], np.int64)
        assert lib.rmu_hybrid_set_keys(h, 0, 0, keys.ctypes.data, 3) == 0
        assert lib.rmu_hybrid_set_keys(h, 1, 0, keys.ctypes.data, 1) == 0                  # a dense table without a dense member
        assert rc() == -1
        assert b"out of step" in lib.rmu_last_error() and b"dense" in lib.rmu_last_error()
    finally:
        lib.rmu_hybrid_free(h)
        lib.rmu_bm25_free(sparse)


def test_equal_texts_share_a_key_numbered_in_first_seen_order():
    from ragmeup_amd.hybrid import content_keys
    classes: dict = {}
    assert content_keys(["b", "a", "b", "", "a", "c"], classes).tolist() == [0, 1, 0, 2, 1, 3]
    assert content_keys([], classes).tolist() == [] and content_keys([], classes).dtype == np.int64
    # the other member draws from the same classes: texts seen before keep their keys, new ones continue the numbering
    assert content_keys(["c", "d", "b", "d"], classes).tolist() == [3, 4, 0, 4]
    assert classes == {"b": 0, "a": 1, "": 2, "c": 3, "d": 4}
    assert content_keys(["A", "a", "a "], {}).tolist() == [0, 1, 2]                       # page_content is compared as it is
