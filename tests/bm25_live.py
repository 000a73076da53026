"""What tests/test_bm25_live_*.py share: a BM25 index with removed documents (include/rmu.h, "Live documents") is checked against the fp64
restatement of tests/bm25_ref.py built over the LIVE texts in id order, with the returned ids mapped through the live list.  The bound is
bm25_ref.scores_tol's -- the arithmetic is the same -- and all three properties of check_topk are asked for: the exact answer satisfies them.

A filtered search (rmu_bm25_search_subset) restricts the candidates and leaves the statistics the live corpus's: `check_subset` asks the same
three properties of the candidates' rows of the same reference."""
from __future__ import annotations

import numpy as np

from tests.bm25_ref import BM25Ref, check_topk

OPT_TILE, OPT_WGS, OPT_REPACK = 1, 2, 4


class LiveCorpus:
    """texts + liveness, and (lazily, per state) the reference over the live texts"""

    def __init__(self, texts):
        self.texts = list(texts)
        self.alive = np.ones(len(self.texts), bool)
        self._ref = None

    def add(self, texts):
        self.texts += list(texts)
        self.alive = np.concatenate([self.alive, np.ones(len(texts), bool)])
        self._ref = None

    def remove(self, ids) -> int:
        ids = np.unique(np.asarray(ids, np.int64))
        n = int(self.alive[ids].sum())
        self.alive[ids] = False
        self._ref = None
        return n

    def compact(self) -> np.ndarray:
        """the map rmu_bm25_compact must hand back"""
        m = np.where(self.alive, np.cumsum(self.alive) - 1, -1).astype(np.int64)
        self.texts = [t for t, a in zip(self.texts, self.alive) if a]
        self.alive = np.ones(len(self.texts), bool)
        self._ref = None
        return m

    @property
    def live_ids(self) -> np.ndarray:
        return np.flatnonzero(self.alive).astype(np.int64)

    @property
    def live_texts(self) -> list:
        return [t for t, a in zip(self.texts, self.alive) if a]

    @property
    def ref(self) -> BM25Ref:
        if self._ref is None:
            self._ref = BM25Ref(self.live_texts)
        return self._ref


def to_positions(ids, docs, doc_base: int = 0) -> np.ndarray:
    """returned document ids -> positions in the ascending list `ids` (+ doc_base again, so that check_topk can take it off); every returned
    id must be in the list; -1 stays -1.  The map is monotone, so the order of ties is checked on the positions as well as on the ids."""
    ids, docs = np.asarray(ids, np.int64), np.asarray(docs, np.int64)
    out = docs.copy()
    real = docs != -1
    got = docs[real] - doc_base
    pos = np.searchsorted(ids, got)
    assert np.all(pos < len(ids)) and np.array_equal(ids[np.minimum(pos, max(len(ids) - 1, 0))], got), (got, "not among the candidates")
    out[real] = pos + doc_base
    return out


def check_live(corpus: LiveCorpus, query: str, scores, docs, k: int, doc_base: int = 0):
    check_topk(corpus.ref, query, scores, to_positions(corpus.live_ids, docs, doc_base), k, doc_base=doc_base)


class _Rows:
    """the candidates' rows of a reference: what check_topk reads (n, scores_tol)"""

    def __init__(self, ref: BM25Ref, rows):
        self.ref, self.rows, self.n = ref, np.asarray(rows, np.int64), len(rows)

    def scores_tol(self, query):
        s, tol = self.ref.scores_tol(query)
        return s[self.rows], tol[self.rows]


def check_subset(corpus: LiveCorpus, allow, query: str, scores, docs, k: int, doc_base: int = 0):
    """candidates = the live documents of `allow` (ascending ids); statistics = the whole live corpus's"""
    allow = np.asarray(allow, np.int64)
    cand = allow[corpus.alive[allow]] if len(allow) else allow
    rows = np.searchsorted(corpus.live_ids, cand)            # the candidates' rows in the reference over the live texts
    check_topk(_Rows(corpus.ref, rows), query, scores, to_positions(cand, docs, doc_base), k, doc_base=doc_base)


def check_all(ix, corpus: LiveCorpus, queries, ks, allow=None, **kw):
    for k in ks:
        s, d = ix.search(queries, k, **({} if allow is None else {"docs": allow}), **kw)
        assert s.shape == (len(queries), k) and s.dtype == np.float32 and d.dtype == np.int64
        for i, q in enumerate(queries):
            if allow is None:
                check_live(corpus, q, s[i], d[i], k, doc_base=kw.get("doc_base", 0))
            else:
                check_subset(corpus, allow, q, s[i], d[i], k, doc_base=kw.get("doc_base", 0))
    return s, d


def same_bits(a, b) -> bool:
    (sa, da), (sb, db) = a, b
    return np.array_equal(sa.view(np.uint32), sb.view(np.uint32)) and np.array_equal(da, db)
