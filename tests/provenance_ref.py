"""Restatement of the reference's similarity provenance (server/provenance.py:164-202) in plain fp64 numpy, for the tests: written from the
definition, independent of ragmeup_amd/provenance.py, which it never imports.

  s_i = cos(doc_i, answer), or (cos(doc_i, answer) + cos(doc_i, query)) / 2 with a query; a NaN / Inf cosine (a zero row) counts as 0
  T = s_0 + s_1 + ... left to right from 0.0;  scores = s_i / T if T > 0 else s_i
"""
from __future__ import annotations

import numpy as np


def cosine(a, b):
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    with np.errstate(all="ignore"):
        sim = np.dot(a, b) / (np.linalg.norm(a) * np.linalg.norm(b))
    if np.isnan(sim) or np.isinf(sim):
        return 0.0
    return float(sim)


def attribute(docs, answer, query=None):
    """docs [n, dim], answer [dim], query [dim] or None -> (scores [n], sims [n, 2], T), float64."""
    docs = np.asarray(docs, dtype=np.float64)
    n = docs.shape[0]
    sims = np.zeros((n, 2), np.float64)
    s = np.zeros(n, np.float64)
    total = 0.0
    for i in range(n):
        sims[i, 0] = cosine(docs[i], answer)
        if query is not None:
            sims[i, 1] = cosine(docs[i], query)
            s[i] = (sims[i, 0] + sims[i, 1]) / 2
        else:
            s[i] = sims[i, 0]
        total = total + s[i]
    scores = s / total if total > 0 else s.copy()
    return scores, sims, total


def attribute_groups(x, groups):
    """The packed outputs of a group table [g, 4] (answer_row, query_row or -1, first_doc_row, n_docs) over the rows of x
    -> (scores, sims, T per group)."""
    x = np.asarray(x)
    scores, sims, totals = [], [], []
    for a, q, first, n in np.asarray(groups).reshape(-1, 4):
        sc, si, t = attribute(x[first:first + n], x[a], x[q] if q >= 0 else None)
        scores.append(sc)
        sims.append(si)
        totals.append(t)
    if not scores:
        return np.empty(0), np.empty((0, 2)), []
    return np.concatenate(scores), np.concatenate(sims), totals


def request_rows(requests, include_query):
    """(query, context, answer) per request -> the texts a batched call embeds, in order, and the group of each request with contexts."""
    texts, groups = [], []
    for query, context, answer in requests:
        if len(context) == 0:
            continue
        row_a = len(texts)
        texts += [answer]
        row_q = -1
        if include_query:
            row_q = len(texts)
            texts += [query]
        groups.append([row_a, row_q, len(texts), len(context)])
        texts += list(context)
    return texts, groups
