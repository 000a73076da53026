"""BM25 on the device: the sparse member of the reference's retrieval ensemble.

The reference builds ``BM25Retriever.from_texts(...)`` (langchain-community over rank_bm25: a Python loop over every document per
query token, an argsort of all N scores, rebuilt from scratch after every upload -- server/RAGHelper.py:436-443, :492-505, :529-531) and
fuses it with the dense retriever.  ``BM25Index`` is the handle on librmu's inverted index in HBM (include/rmu.h, bm25.hip);
``MI355XBM25Retriever`` carries langchain's BM25Retriever surface over it, plus incremental ``add_documents`` / ``add_texts`` and
``batch_invoke`` (one search for a batch, which ``MI355XEnsembleRetriever.batch_invoke`` looks for).

Scores are rank_bm25.BM25Okapi's.  Ties: score descending, then the LOWER document id -- rank_bm25's ``argsort()[::-1]`` puts the higher
id first among equal scores and is not stable.  Not provided: deleting documents, persistence, the ParadeDB SQL retriever.
"""
from __future__ import annotations

import ctypes
from typing import Any, Callable, Iterable, List, Optional

import numpy as np

from . import _native as N
from ._lc import BaseRetriever, Document


def _blob(texts: list[str]) -> bytes:
    """n strings -> one NUL-separated UTF-8 blob (the convention of rmu_tok_encode_blob)."""
    for t in texts:
        if "\0" in t:
            raise ValueError("a text holds U+0000, which separates the texts on their way into the library")
    return ("\0".join(texts) + "\0").encode("utf-8", "surrogatepass") if texts else b""


class BM25Index:
    """Okapi BM25 inverted index: postings on the host, one packed image in HBM, fused score + top-k on the device."""

    def __init__(self, k1: float = 1.5, b: float = 0.75, epsilon: float = 0.25):
        self._lib = N.lib()
        h = ctypes.c_void_p()
        N.check(self._lib.rmu_bm25_create(ctypes.byref(h), float(k1), float(b), float(epsilon)), "rmu_bm25_create")
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            self._lib.rmu_bm25_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def add_texts(self, texts: Iterable[str]) -> int:
        """Append documents (host only; the next search uploads the image); returns the id of the first one."""
        texts = list(texts)
        blob = _blob(texts)
        first = ctypes.c_int64()
        N.check(self._lib.rmu_bm25_add_texts(self._h, blob, len(blob), len(texts), ctypes.byref(first)), "rmu_bm25_add_texts")
        return int(first.value)

    def stat(self) -> dict:
        out = {}
        for name, what in (("docs", N.BM25_STAT_DOCS), ("vocab", N.BM25_STAT_VOCAB), ("nnz", N.BM25_STAT_NNZ), ("avgdl", N.BM25_STAT_AVGDL)):
            v = ctypes.c_double()
            N.check(self._lib.rmu_bm25_stat(self._h, what, ctypes.byref(v)), "rmu_bm25_stat")
            out[name] = float(v.value) if name == "avgdl" else int(v.value)
        return out

    def __len__(self) -> int:
        return self.stat()["docs"]

    def df(self, term: str) -> int:
        v = ctypes.c_int64()
        N.check(self._lib.rmu_bm25_df(self._h, term.encode("utf-8", "surrogatepass"), ctypes.byref(v)), "rmu_bm25_df")
        return int(v.value)

    def set_option(self, option: int, value: int):
        N.check(self._lib.rmu_bm25_set_option(self._h, int(option), int(value)), "rmu_bm25_set_option")

    def search(self, queries: list[str], k: int, doc_base: int = 0, stream: int = 0):
        """(scores [nq, k] float32, docs [nq, k] int64), best first; slots beyond the corpus hold (-inf, -1)."""
        queries = list(queries)
        nq = len(queries)
        scores = np.empty((nq, int(k)), np.float32)
        docs = np.empty((nq, int(k)), np.int64)
        if nq == 0:
            return scores, docs
        blob = _blob(queries)
        N.check(self._lib.rmu_bm25_search(self._h, blob, len(blob), nq, int(k), int(doc_base), scores.ctypes.data, docs.ctypes.data,
                                          int(stream)), "rmu_bm25_search")
        return scores, docs


def _joined(tokens) -> str:
    """Tokens of a caller's preprocess_func -> the text whose str.split() gives them back."""
    toks = list(tokens)
    for t in toks:
        if not isinstance(t, str) or not t or any(ch.isspace() for ch in t):
            raise ValueError(f"preprocess_func returned {t!r}: every token must be a non-empty string without whitespace")
    return " ".join(toks)


class MI355XBM25Retriever(BaseRetriever):
    """``BM25Retriever`` (langchain-community) over ``BM25Index``: fields ``vectorizer`` (the index), ``docs``, ``k`` and
    ``preprocess_func`` (None = str.split(), langchain's default, done inside the library)."""

    vectorizer: Any = None
    docs: List[Any] = []
    k: int = 4
    preprocess_func: Optional[Callable[[str], List[str]]] = None

    class Config:
        arbitrary_types_allowed = True

    def _text(self, text: str) -> str:
        return text if self.preprocess_func is None else _joined(self.preprocess_func(text))

    @classmethod
    def from_texts(cls, texts: Iterable[str], metadatas: Optional[Iterable[dict]] = None, ids: Optional[Iterable[str]] = None,
                   bm25_params: Optional[dict] = None, preprocess_func: Optional[Callable[[str], List[str]]] = None, **kwargs: Any):
        self = cls(vectorizer=BM25Index(**(bm25_params or {})), docs=[], preprocess_func=preprocess_func, **kwargs)
        self.add_texts(texts, metadatas, ids=ids)
        return self

    @classmethod
    def from_documents(cls, documents: Iterable[Document], *, bm25_params: Optional[dict] = None,
                       preprocess_func: Optional[Callable[[str], List[str]]] = None, **kwargs: Any):
        documents = list(documents)
        return cls.from_texts([d.page_content for d in documents], [d.metadata for d in documents],
                              [getattr(d, "id", None) for d in documents], bm25_params, preprocess_func, **kwargs)

    def add_texts(self, texts: Iterable[str], metadatas: Optional[Iterable[dict]] = None, ids: Optional[Iterable[str]] = None) -> list:
        texts = list(texts)
        metadatas = list(metadatas) if metadatas is not None else [{} for _ in texts]
        ids = list(ids) if ids is not None else [None] * len(texts)
        if not (len(texts) == len(metadatas) == len(ids)):
            raise ValueError("texts, metadatas and ids differ in length")
        prepared = [self._text(t) for t in texts]
        first = self.vectorizer.add_texts(prepared)
        assert first == len(self.docs)
        for t, m, i in zip(texts, metadatas, ids):
            d = Document(page_content=t, metadata=dict(m or {}))
            if i is not None:
                try:
                    d.id = i
                except (AttributeError, ValueError):   # a Document type without an id
                    pass
            self.docs.append(d)
        return ids

    def add_documents(self, documents: Iterable[Document], ids: Optional[Iterable[str]] = None) -> list:
        """Incremental upload (the reference rebuilds the whole retriever instead, RAGHelper.py:529-531)."""
        documents = list(documents)
        return self.add_texts([d.page_content for d in documents], [d.metadata for d in documents],
                              ids if ids is not None else [getattr(d, "id", None) for d in documents])

    def batch_invoke(self, queries: list[str]) -> list[list[Document]]:
        """One rmu_bm25_search for the whole batch."""
        queries = list(queries)
        if not queries or not self.docs:
            return [[] for _ in queries]
        _, rows = self.vectorizer.search([self._text(q) for q in queries], min(int(self.k), N.MAX_K))
        return [[self.docs[r] for r in row if r >= 0] for row in rows.tolist()]

    def _get_relevant_documents(self, query: str, *, run_manager: Any = None, **kw) -> list[Document]:
        return self.batch_invoke([query])[0]
