"""Restatement of langchain_experimental 0.0.64's SemanticChunker in plain numpy and Python, for the tests: written from the definition
(sentence split, windows, cosine distances, the four thresholds and the number_of_chunks map, chunk assembly), independent of
ragmeup_amd/chunker.py, which it never imports.

`params` everywhere: {"type": ..., "amount": None | number, "number_of_chunks": None | int}.
"""
from __future__ import annotations

import hashlib
import random
import re

import numpy as np

SPLIT = r"(?<=[.?!])\s+"
DEFAULT_AMOUNT = {"percentile": 95, "standard_deviation": 3, "interquartile": 1.5, "gradient": 95}


def sentences_of(text, regex=SPLIT):
    return re.split(regex, text)


def windows_of(sentences, buffer_size=1):
    out = []
    for i in range(len(sentences)):
        before = [sentences[j] + " " for j in range(i - buffer_size, i) if j >= 0]
        after = [" " + sentences[j] for j in range(i + 1, i + 1 + buffer_size) if j < len(sentences)]
        out.append("".join(before) + sentences[i] + "".join(after))
    return out


def embedded(sentences, params):
    if len(sentences) == 1:
        return False
    if params["type"] == "gradient" and len(sentences) == 2:
        return False
    return True


def distances(E):
    """1 - cosine of adjacent rows, float64; a NaN / Inf similarity counts as 0."""
    E = np.asarray(E, dtype=np.float64)
    out = np.empty(max(E.shape[0] - 1, 0), np.float64)
    with np.errstate(all="ignore"):
        for i in range(E.shape[0] - 1):
            a, b = E[i], E[i + 1]
            sim = np.dot(a, b) / (np.linalg.norm(a) * np.linalg.norm(b))
            if np.isnan(sim) or np.isinf(sim):
                sim = 0.0
            out[i] = 1.0 - sim
    return out


def threshold_of(d, params):
    """-> (threshold, compared array)"""
    if params.get("number_of_chunks") is not None:
        x1 = len(d)
        x = max(min(params["number_of_chunks"], x1), 1.0)
        if x1 == 1:
            y = 100.0
        else:
            y = 0.0 + (100.0 / (1.0 - x1)) * (x - x1)
        y = min(max(y, 0), 100)
        return np.percentile(d, y), d
    kind = params["type"]
    amount = params.get("amount")
    if amount is None:
        amount = DEFAULT_AMOUNT[kind]
    if kind == "percentile":
        return np.percentile(d, amount), d
    if kind == "standard_deviation":
        return np.mean(d) + amount * np.std(d), d
    if kind == "interquartile":
        q1, q3 = np.percentile(d, [25, 75])
        return np.mean(d) + amount * (q3 - q1), d
    if kind == "gradient":
        g = np.gradient(d, range(len(d)))
        return np.percentile(g, amount), g
    raise ValueError(kind)


def margin_of(d, params):
    """min |array[i] - thr| over the entries that are not bit-equal to thr (inf when there is none)."""
    thr, arr = threshold_of(d, params)
    gaps = [abs(v - thr) for v in arr if v != thr]
    return min(gaps) if gaps else float("inf")


def chunks_from_distances(sentences, d, params):
    if not embedded(sentences, params):
        return list(sentences)
    thr, arr = threshold_of(d, params)
    chunks, start = [], 0
    for i in range(len(arr)):
        if arr[i] > thr:
            chunks.append(" ".join(sentences[start:i + 1]))
            start = i + 1
    if start < len(sentences):
        chunks.append(" ".join(sentences[start:]))
    return chunks


def split_text(text, embed, params, buffer_size=1, regex=SPLIT):
    """The whole splitter over `embed(list of texts) -> [n, dim] array`."""
    s = sentences_of(text, regex)
    if not embedded(s, params):
        return list(s)
    return chunks_from_distances(s, distances(embed(windows_of(s, buffer_size))), params)


# ---- the stub embedding and the documents of the GPU tests -------------------------------------------------------------------------------
_WORD_CACHE: dict = {}


def word_vector(word, dim):
    key = (word, dim)
    v = _WORD_CACHE.get(key)
    if v is None:
        seed = int.from_bytes(hashlib.md5(word.encode("utf-8")).digest()[:8], "little")
        v = _WORD_CACHE[key] = np.random.default_rng(seed).standard_normal(dim)
    return v


def stub_embed(texts, dim):
    """fp32 of the normalised sum over text.split() of a Gaussian seeded by the word's md5 (a text without words: the zero vector)."""
    out = np.zeros((len(texts), dim), np.float32)
    for i, t in enumerate(texts):
        words = t.split()
        if not words:
            continue
        s = np.sum([word_vector(w, dim) for w in words], axis=0)
        out[i] = (s / np.linalg.norm(s)).astype(np.float32)
    return out


def make_document(n_sentences, seed):
    """n sentences of 3-11 words t{topic}w{j} from 5 topics of 40 words, each ending in '.', '?' or '!'; the topic changes with
    probability 0.15 per sentence."""
    rng = random.Random(seed * 1000003 + n_sentences)
    topic = rng.randrange(5)
    sents = []
    for _ in range(n_sentences):
        if rng.random() < 0.15:
            topic = rng.choice([t for t in range(5) if t != topic])
        words = [f"t{topic}w{rng.randrange(40)}" for _ in range(rng.randint(3, 11))]
        sents.append(" ".join(words) + rng.choice(".?!"))
    return " ".join(sents)
