"""Host restatement of csrc/rerank.hip: the assembly of a (query, passage) pair and the stable top-n (tests only)."""
from __future__ import annotations

import math

import numpy as np


def longest_first(len1: int, len2: int, budget: int) -> tuple[int, int]:
    """Tokens the two sides keep, stated as the rule reads (not as the library computes it): nothing is cut when both fit; only the longer
    side when that suffices; otherwise both go to half the budget, the odd token to the longer side, to the second on equal lengths."""
    if len1 + len2 <= budget:
        return len1, len2
    short, long_ = min(len1, len2), max(len1, len2)
    if short <= budget - short:                      # cutting the longer side alone suffices (it stays at least as long as the shorter)
        keep_short, keep_long = short, budget - short
    else:
        keep_short, keep_long = budget // 2, budget - budget // 2
    if len1 > len2:
        return keep_long, keep_short
    return keep_short, keep_long                     # (equal lengths: the second side is "the longer")


def assemble(q_tok, p_tok, max_len: int, cls: int, sep: int, pad: int):
    """-> (ids [max_len], types [max_len], length) of [CLS] q [SEP] p [SEP] [PAD]...; q_tok / p_tok: the two texts' tokens WITHOUT special
    tokens and before any cut; p_tok None: an absent passage (key -1), a row of [PAD] with length 0."""
    ids = np.full(max_len, pad, dtype=np.int32)
    types = np.zeros(max_len, dtype=np.int32)
    if p_tok is None:
        return ids, types, 0
    n1, n2 = longest_first(len(q_tok), len(p_tok), max_len - 3)
    row = [cls] + list(q_tok[:n1]) + [sep] + list(p_tok[:n2]) + [sep]
    ids[:len(row)] = row
    types[n1 + 2:len(row)] = 1
    return ids, types, len(row)


def select(logits, keys, top_n: int):
    """-> (positions [top_n] int32, scores [top_n] fp32) of one query: Python's stable sorted(reverse=True) over the present candidates
    (key >= 0); a NaN behind every number, NaNs among themselves by position; the slots past the present candidates hold (-1, -inf)."""
    logits = np.asarray(logits, dtype=np.float32)
    present = [(i, float(logits[i])) for i in range(len(logits)) if keys[i] >= 0]
    # (+0.0 == -0.0 as Python compares them; a reverse sort keeps equal elements in their original order)
    ranked = sorted(present, key=lambda e: (0, 0.0) if math.isnan(e[1]) else (1, e[1]), reverse=True)[:top_n]
    pos = np.full(top_n, -1, dtype=np.int32)
    scores = np.full(top_n, -np.inf, dtype=np.float32)
    for slot, (i, _) in enumerate(ranked):
        pos[slot] = i
        scores[slot] = logits[i]
    return pos, scores


def grid(max_len: int) -> list[int]:
    """The lengths on both sides of every edge of the rule at this max_len."""
    b = max_len - 3
    return sorted({0, 1, b // 2 - 1, b // 2, b // 2 + 1, b - 1, b, b + 1, 2 * b})
