"""The grouped search (rmu_index_search_distinct, ragmeup_amd/csrc/scan_distinct.hip) restated on the host, numpy only: rank every live row
with the chain scores of tests/exact_regimes.py -- the bits rmu_index_search gives -- in its order (score descending, then lower row id),
walk that order and keep a row iff no kept row has its code, stop at k.  Plus the planner of the distinct scan, so that a test can put rows
on both sides of its tile, workgroup-chunk and row-part boundaries.

A plain helper module, not a fixture: tests/test_distinct_cpu.py holds it to a hand-written case, tests/test_distinct_gpu.py holds the
library to it bit for bit."""
from __future__ import annotations

import numpy as np

from tests import exact_regimes as E

MAX_K = 32                         # RMU_MAX_K_DISTINCT
NQ_W1 = 32                         # wq = nq <= 32 ? 1 : 4


def plan(n: int, nq: int) -> dict:
    """rmu_distinct_plan: the geometry of one launch over n rows and nq <= 8192 queries"""
    wq = 1 if nq <= NQ_W1 else 4
    rp = 4 // wq
    rt = 32 * rp
    nqt = (nq + 32 * wq - 1) // (32 * wq)
    tiles_total = (n + rt - 1) // rt
    s_chunks, tpc = E.plan_chunks(nqt, tiles_total)
    return dict(wq=wq, RT=rt, RP=rp, nqt=nqt, tiles_total=tiles_total, s_chunks=s_chunks, tiles_per_chunk=tpc, grid=s_chunks * nqt,
                parts=s_chunks * rp, chunk_rows=tpc * rt)


def walk(rs, rr, codes, k: int) -> tuple:
    """(scores, rows) [nq, <= k] ranked best first over ALL live rows (padded with (-inf, -1)) -> the first k rows per query whose code no
    earlier kept row has, padded the same way"""
    nq = rs.shape[0]
    out_s = np.full((nq, k), -np.inf, np.float32)
    out_r = np.full((nq, k), -1, np.int64)
    for i in range(nq):
        live = int((rr[i] >= 0).sum())                          # (the padding comes last)
        # greedy walk = the first occurrence of every code in the ranked order, the earliest k of them
        _, first = np.unique(codes[rr[i, :live]], return_index=True)
        keep = np.sort(first)[:k]
        out_s[i, :keep.size], out_r[i, :keep.size] = rs[i, keep], rr[i, keep]
    return out_s, out_r


def distinct_from_scores(scores, alive, codes, k: int, qn2=None, row_base: int = 0) -> tuple:
    """scores [nq, n]: the scan's scores (chain bits).  -> what rmu_index_search_distinct returns: (scores, rows) [nq, k]"""
    scores = np.asarray(scores, np.float32)
    rs, rr = E.ranked(scores, alive, scores.shape[1])          # every live row, in rmu_index_search's order
    ds, dr = walk(rs, rr, np.asarray(codes), k)
    out_s, out_r = E.topk_from_order(ds, dr, k, qn2)            # the L2 distances and the padding as the library's
    return out_s, np.where(out_r >= 0, out_r + row_base, -1)


def chain_scores(metric: str, q, x, dim: int, dpad: int) -> tuple:
    """(chain scores [nq, n], |q|^2 or None) of an index of this metric holding rows x, for queries q"""
    qi, xi, qn2 = E.images(metric, q, x, dim, dpad)
    return E.chain(qi, xi, dpad), qn2


def search_distinct(metric: str, q, x, codes, k: int, dim: int, dpad: int, alive=None, row_base: int = 0) -> tuple:
    s, qn2 = chain_scores(metric, q, x, dim, dpad)
    return distinct_from_scores(s, alive, codes, k, qn2, row_base)
