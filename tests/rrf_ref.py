"""Weighted reciprocal-rank fusion in pure Python, with what rmu_rrf_fuse reports beside the order: the fp64 score of every fused key and the
(list, position) of the entry that represents it (include/rmu.h, "hybrid retrieval").  Absent slots (-1) may stand anywhere in a list and
consume no rank.  Every call checks its own order against oracle.weighted_rrf over the lists with the absent slots taken out."""
from __future__ import annotations

import numpy as np

from oracle import oracle as O


def fuse(lists, weights, c: int = 60):
    """lists: one sequence of int keys per list (best first, -1 = absent).  -> (keys, scores, src): the distinct keys by score descending,
    equal scores in first-seen (chain) order; scores as Python floats; src[i] = (list, position) of the first entry holding keys[i]."""
    score: dict = {}
    first: dict = {}
    for l, (lst, w) in enumerate(zip(lists, weights)):
        rank = 0
        for pos, key in enumerate(lst):
            key = int(key)
            if key < 0:
                continue
            rank += 1
            if key not in score:
                score[key] = 0.0
                first[key] = (l, pos)
            score[key] += w / (rank + c)
    keys = sorted(score, key=lambda k: score[k], reverse=True)          # stable: dict order is first-seen order
    assert keys == O.weighted_rrf([[int(k) for k in lst if k >= 0] for lst in lists], list(weights), c)
    return keys, [score[k] for k in keys], [first[k] for k in keys]


def fuse_arrays(keys: np.ndarray, weights, c: int, k_out: int):
    """The arrays rmu_rrf_fuse returns for keys [lists, nq, depth]: (scores [nq, k_out] float64, keys [nq, k_out] int64, src [nq, k_out]
    int32 = list * depth + position), padded with (-inf, -1, -1)."""
    lists, nq, depth = keys.shape
    s = np.full((nq, k_out), -np.inf, np.float64)
    k = np.full((nq, k_out), -1, np.int64)
    r = np.full((nq, k_out), -1, np.int32)
    for q in range(nq):
        kk, ss, src = fuse([keys[l, q].tolist() for l in range(lists)], weights, c)
        m = min(k_out, len(kk))
        s[q, :m] = ss[:m]
        k[q, :m] = kk[:m]
        r[q, :m] = [l * depth + p for l, p in src[:m]]
    return s, k, r


def random_case(rng, lists: int, nq: int, depth: int):
    """keys [lists, nq, depth]: a universe of about lists * depth / 2 keys (overlaps are the rule), a third of the lists drawn with
    repetition, absent tails of random length, a few absent slots in the middle, one all-absent list and one all-absent query (where that leaves something)."""
    universe = max(2, lists * depth // 2)
    keys = np.full((lists, nq, depth), -1, np.int64)
    for l in range(lists):
        for q in range(nq):
            n = int(rng.integers(0, depth + 1))
            if rng.integers(0, 3) == 0 or n > universe:
                keys[l, q, :n] = rng.integers(0, universe, n)
            else:
                keys[l, q, :n] = rng.choice(universe, n, replace=False)
            if n > 2 and rng.integers(0, 4) == 0:
                keys[l, q, rng.integers(0, n, max(1, n // 8))] = -1
    if lists > 1 or nq > 1:
        keys[int(rng.integers(0, lists)), int(rng.integers(0, nq))] = -1
    if nq > 1:
        keys[:, int(rng.integers(0, nq))] = -1
    return keys
