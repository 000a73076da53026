"""fp64 host restatement of Okapi BM25 as rank_bm25.BM25Okapi computes it under langchain's BM25Retriever, written from the formula
(include/rmu.h, "BM25 retriever"), plus the synthetic corpora and the checks tests/test_bm25_*.py share.

    tokens = str.split();  idf[t] = ln(N - df + 0.5) - ln(df + 0.5), idf < 0 -> epsilon * mean(idf before replacement)
    score(q, d) = sum over q's tokens in order of idf[t] * tf * (k1 + 1) / (tf + k1 * (1 - b + b * dl[d] / avgdl))
"""
from __future__ import annotations

from collections import Counter

import numpy as np

# every code point str.isspace() accepts
WHITESPACE = ([chr(c) for c in range(0x09, 0x0E)] + [chr(c) for c in range(0x1C, 0x20)] + [" ", "\x85", "\xa0", "\u1680"]
              + [chr(c) for c in range(0x2000, 0x200B)] + ["\u2028", "\u2029", "\u202f", "\u205f", "\u3000"])
assert all(c.isspace() for c in WHITESPACE) and len(WHITESPACE) == sum(chr(c).isspace() for c in range(0x110000))


class BM25Ref:
    def __init__(self, texts, k1=1.5, b=0.75, epsilon=0.25):
        self.k1, self.b, self.epsilon = float(k1), float(b), float(epsilon)
        self.n = len(texts)
        toks = [t.split() for t in texts]
        self.dl = np.array([len(t) for t in toks], np.float64)
        self.avgdl = float(self.dl.sum() / self.n) if self.n else 0.0
        post: dict[str, tuple[list, list]] = {}
        for d, t in enumerate(toks):
            for term, tf in Counter(t).items():
                e = post.setdefault(term, ([], []))
                e[0].append(d)
                e[1].append(tf)
        self.post = {t: (np.array(a, np.int64), np.array(f, np.float64)) for t, (a, f) in post.items()}
        self.df = {t: len(a) for t, (a, _) in self.post.items()}
        self.nnz = sum(self.df.values())
        idf = {t: float(np.log(self.n - df + 0.5) - np.log(df + 0.5)) for t, df in self.df.items()}
        mean = sum(idf.values()) / len(idf) if idf else 0.0
        self.idf = {t: (self.epsilon * mean if v < 0 else v) for t, v in idf.items()}
        self._cache: dict = {}

    def contributions(self, query: str) -> np.ndarray:
        """[T, N] fp64: c_t(q, d) per query token (zero rows for unknown tokens)."""
        toks = query.split()
        c = np.zeros((len(toks), self.n), np.float64)
        for i, t in enumerate(toks):
            if t in self.post:
                docs, tf = self.post[t]
                c[i, docs] = self.idf[t] * tf * (self.k1 + 1.0) / (tf + self.k1 * (1.0 - self.b + self.b * self.dl[docs] / self.avgdl))
        return c

    def scores_tol(self, query: str):
        """(fp64 scores [N], tol [N]): tol(q, d) = (T + 8) * 2^-23 * sum_t |c_t(q, d)|, the bound on the library's fp32 score: the idf and
        doc_norm roundings, the multiply, the add and the correctly rounded divide give at most 8 half-ulps per contribution (hipcc's fp32
        divide is correctly rounded by default: -fhip-fp32-correctly-rounded-divide-sqrt), the ordered sum at most one per addition."""
        if query not in self._cache:
            c = self.contributions(query)
            s = np.zeros(self.n, np.float64)
            for row in c:                       # in query order
                s = s + row
            self._cache[query] = (s, (c.shape[0] + 8) * 2.0 ** -23 * np.abs(c).sum(axis=0))
        return self._cache[query]


def check_topk(ref: BM25Ref, query: str, scores, docs, k: int, doc_base: int = 0):
    """Properties 1-3 of one result row (scores fp32 [k], docs int64 [k])."""
    scores, docs = np.asarray(scores), np.asarray(docs)
    assert scores.shape == (k,) and docs.shape == (k,)
    s64, tol = ref.scores_tol(query)
    m = min(k, ref.n)
    got = docs[:m] - doc_base
    assert np.all(docs[m:] == -1) and np.all(np.isneginf(scores[m:])), (docs, scores)
    assert np.all((got >= 0) & (got < ref.n)) and len(set(got.tolist())) == m, docs
    # 1. every returned score is the fp64 score of that document up to the derived rounding bound
    err = np.abs(scores[:m].astype(np.float64) - s64[got])
    assert np.all(err <= tol[got]), (query, err.max(), got[np.argmax(err - tol[got])])
    # 2. ordered by (returned score descending, document id ascending)
    for i in range(m - 1):
        assert scores[i] > scores[i + 1] or (scores[i] == scores[i + 1] and got[i] < got[i + 1]), (query, i, scores[i:i + 2], got[i:i + 2])
    # 3. nothing left out beats the last returned document by more than the bound (of either of the two)
    if m < ref.n:
        out = np.ones(ref.n, bool)
        out[got] = False
        last = got[m - 1]
        over = s64[out] - s64[last] - np.maximum(tol[out], tol[last])
        assert over.max() <= 0.0, (query, over.max())


def synth_corpus(n: int, seed: int = 0, vocab: int = 500, lmax: int = 60, every: str | None = None) -> list[str]:
    """n documents of 0..lmax words drawn Zipf-like from `vocab` synthetic words (w0 most frequent); `every`: a word put into every document."""
    rng = np.random.default_rng(seed)
    p = 1.0 / np.arange(1, vocab + 1)
    p /= p.sum()
    lens = rng.integers(0, lmax + 1, n)
    words = rng.choice(vocab, int(lens.sum()), p=p)
    out, at = [], 0
    for l in lens:
        w = [f"w{i}" for i in words[at:at + l]]
        at += l
        if every is not None:
            w.insert(len(w) // 2, every)
        out.append(" ".join(w))
    return out


def synth_queries(texts: list[str], n: int, seed: int = 1, tmin: int = 1, tmax: int = 12) -> list[str]:
    """n queries of tmin..tmax words sampled from the corpus' own words (so frequent words are frequent in queries too)."""
    rng = np.random.default_rng(seed)
    pool = " ".join(texts).split() or ["w0"]
    return [" ".join(pool[i] for i in rng.integers(0, len(pool), rng.integers(tmin, tmax + 1))) for _ in range(n)]
