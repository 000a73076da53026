"""ctypes loader for the plain-C oracle (oracle/flat_search.c).  TEST INFRASTRUCTURE ONLY."""
from __future__ import annotations

import ctypes
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_SO = os.path.join(_HERE, "_build", "liboracle_flat.so")
_lib = None


def build(force: bool = False) -> str:
    src = os.path.join(_HERE, "flat_search.c")
    if force or not os.path.exists(_SO) or os.path.getmtime(_SO) < os.path.getmtime(src):
        # -march=native is unsafe for a .so that travels to another box: build generic x86-64-v3
        subprocess.check_call(["make", "-C", _HERE, "-s",
                               "CFLAGS=-O3 -mavx2 -mfma -fopenmp -fPIC -std=c11 -Wall -Wextra"])
    return _SO


def lib():
    global _lib
    if _lib is None:
        build()                      # (a library older than its source lacks what the source has gained)
        _lib = ctypes.CDLL(_SO)
        _lib.oracle_flat_search.restype = ctypes.c_int
        _lib.oracle_flat_search.argtypes = [
            ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int,
            ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
        _lib.oracle_num_threads.restype = ctypes.c_int
        for f in (_lib.oracle_chain_scores, _lib.oracle_natural_scores):
            f.restype = ctypes.c_int
            f.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_void_p]
        _lib.oracle_wave_sumsq.restype = ctypes.c_int
        _lib.oracle_wave_sumsq.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    return _lib


def num_threads() -> int:
    return int(lib().oracle_num_threads())


def flat_search(q: np.ndarray, x: np.ndarray, k: int, metric: int = 0, alive: np.ndarray | None = None):
    q = np.ascontiguousarray(q, dtype=np.float32)
    x = np.ascontiguousarray(x, dtype=np.float32)
    nq, d = q.shape
    out_s = np.empty((nq, k), dtype=np.float32)
    out_r = np.empty((nq, k), dtype=np.int64)
    am = None
    if alive is not None:
        am = np.ascontiguousarray(alive, dtype=np.uint8)
    rc = lib().oracle_flat_search(q.ctypes.data, nq, x.ctypes.data, x.shape[0], d, k, metric,
                                  am.ctypes.data if am is not None else None,
                                  out_s.ctypes.data, out_r.ctypes.data)
    if rc != 0:
        raise RuntimeError(f"oracle_flat_search failed: {rc}")
    return out_s, out_r


def _padded(a: np.ndarray, dpad: int) -> np.ndarray:
    a = np.ascontiguousarray(a, dtype=np.float32)
    if a.shape[1] == dpad:
        return a
    out = np.zeros((a.shape[0], dpad), dtype=np.float32)
    out[:, :a.shape[1]] = a
    return out


def chain_scores(q: np.ndarray, x: np.ndarray, dpad: int | None = None, natural: bool = False) -> np.ndarray:
    """fp32 scores [nq, n] as the exact scan's MFMA chain sums them (oracle_chain_scores), bit for bit; `natural`: the same products in
    the order k = 0, 1, 2, ... instead.  q and x are zero-padded to `dpad` columns (default: as wide as they are)."""
    dpad = int(dpad or x.shape[1])
    q, x = _padded(q, dpad), _padded(x, dpad)
    out = np.empty((q.shape[0], x.shape[0]), dtype=np.float32)
    f = lib().oracle_natural_scores if natural else lib().oracle_chain_scores
    rc = f(q.ctypes.data, q.shape[0], x.ctypes.data, x.shape[0], dpad, out.ctypes.data)
    if rc != 0:
        raise RuntimeError(f"oracle_chain_scores failed: {rc}")
    return out


def wave_sumsq(x: np.ndarray, ncols: int | None = None) -> np.ndarray:
    """|row|^2 over the first `ncols` columns as one wave of the image kernels sums it (oracle_wave_sumsq)."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    out = np.empty(x.shape[0], dtype=np.float32)
    rc = lib().oracle_wave_sumsq(x.ctypes.data, x.shape[0], x.shape[1], x.shape[1] if ncols is None else int(ncols), out.ctypes.data)
    if rc != 0:
        raise RuntimeError(f"oracle_wave_sumsq failed: {rc}")
    return out
