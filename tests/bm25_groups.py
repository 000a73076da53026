"""What tests/test_bm25_groups_*.py share (not collected): corpora, the families of document lists and the queries of
rmu_bm25_search_groups (include/rmu.h), and the planner's test hook behind ctypes."""
from __future__ import annotations

import numpy as np

from tests.bm25_ref import synth_corpus, synth_queries

TILE = 64                      # the smallest tile: every corpus below spans several
SIZES = (65, 321, 5000)        # one tile + one document (the last mask word pair lies past N); 5 tiles + 1; many tiles and parts
_TEXTS: dict = {}


def texts_of(n: int) -> list[str]:
    if n not in _TEXTS:
        _TEXTS[n] = synth_corpus(n, seed=n)
    return _TEXTS[n]


def removed_of(n: int) -> np.ndarray:
    """30 % of the documents, the same ones every time; never document 0, so that something is always live"""
    rng = np.random.default_rng(1000 + n)
    return np.sort(rng.choice(np.arange(1, n), (3 * n) // 10, replace=False)).astype(np.int64)


def queries_of(n: int, count: int) -> list[str]:
    """corpus words, plus the empty query and a query of unknown words only"""
    return synth_queries(texts_of(n), max(count - 2, 1), seed=7 + n) + ["", "zz-unknown qq-unknown"]


def case_lists(n: int, removed=None, tile: int = TILE) -> dict:
    """name -> strictly ascending int64 ids in [0, n): the families of the issue.  `removed`: the ids "only_removed" draws from."""
    a = lambda x: np.asarray(x, dtype=np.int64)
    run_lo = min(n - 1, tile + 3)                                       # starts mid-tile, mid-corpus: every cursor comes from the search
    last_tile = (n - 1) // tile * tile
    removed = a([]) if removed is None else a(removed)
    return {
        "run": np.arange(run_lo, min(n, run_lo + 2 * tile + 5), dtype=np.int64),
        "every_7th": np.arange(0, n, 7, dtype=np.int64),
        "one": a([n // 2]),
        "empty": a([]),
        "whole": np.arange(n, dtype=np.int64),
        "only_removed": removed[: max(1, removed.size // 2)] if removed.size else a([]),
        "first_and_last_tile": np.unique(np.concatenate([np.arange(0, min(tile, n)), np.arange(last_tile, n)])).astype(np.int64),
        "overlap_a": np.arange(0, min(n, 3 * tile // 2), dtype=np.int64),
        "overlap_b": np.arange(min(n - 1, tile // 2), min(n, 3 * tile), dtype=np.int64),
        "twice_1": np.arange(1, n, 3, dtype=np.int64),
        "twice_2": np.arange(1, n, 3, dtype=np.int64),
        "unused": np.arange(0, n, 2, dtype=np.int64),
    }


def assignment(names: list[str], nq: int, seed: int = 0) -> np.ndarray:
    """q_list in shuffled order: every list but "unused" gets a query while there are queries, the rest are drawn at random"""
    usable = [i for i, name in enumerate(names) if name != "unused"]
    rng = np.random.default_rng(seed)
    ql = np.asarray([usable[i % len(usable)] for i in range(nq)], dtype=np.int64)
    if nq > len(usable):
        ql[len(usable):] = rng.choice(usable, nq - len(usable))
    rng.shuffle(ql)
    return ql


def plan(lib, n_docs: int, live: np.ndarray, tile: int, cap: int, lists: list, q_list):
    """rmu_bm25_groups_plan_ -> (rc, work [n, 5] int32 = (query, part, d_lo, d_hi, first mask word), mask words uint32,
    counts = (entries, mask words, kept tiles, most parts of a query))"""
    lists = [np.ascontiguousarray(x, dtype=np.int64).reshape(-1) for x in lists]
    ptr = np.zeros(len(lists) + 1, np.int64)
    np.cumsum([x.size for x in lists], out=ptr[1:])
    docs = np.concatenate(lists) if lists else np.zeros(0, np.int64)
    docs = np.ascontiguousarray(np.concatenate([docs, np.zeros(1, np.int64)]))            # (never an empty buffer)
    ql = np.ascontiguousarray(q_list, dtype=np.int32)
    live = np.ascontiguousarray(live, dtype=np.uint8)
    counts = np.zeros(4, np.int64)
    rc = lib.rmu_bm25_groups_plan_(n_docs, live.ctypes.data, tile, cap, docs.ctypes.data, ptr.ctypes.data, len(lists), ql.ctypes.data, ql.size,
                                   None, 0, None, 0, counts.ctypes.data)
    if rc != 0:
        return rc, None, None, counts
    work = np.zeros((int(counts[0]) + 1, 5), np.int32)
    mask = np.zeros(int(counts[1]) + 1, np.uint32)
    rc = lib.rmu_bm25_groups_plan_(n_docs, live.ctypes.data, tile, cap, docs.ctypes.data, ptr.ctypes.data, len(lists), ql.ctypes.data, ql.size,
                                   work.ctypes.data, int(counts[0]), mask.ctypes.data, int(counts[1]), counts.ctypes.data)
    return rc, work[:-1], mask[:-1], counts
