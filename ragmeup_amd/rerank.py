"""Rerank by key -- the host half of csrc/rerank.hip (rmu_passages_*, rmu_bert_rerank).

The reference answers a /chat request by retrieving through the ensemble, reranking through
``ContextualCompressionRetriever(base_compressor=ScoredCrossEncoderReranker, base_retriever=ensemble)`` (server/RAGHelper.py:476-490,
RAGHelper_local.py:157-159) and, for ``provenance_method == "rerank"``, running the same compressor once more with the answer as the query
(server/provenance.py:100-108).  Each pass tokenises every retrieved passage again, although a passage's tokens are a pure function of its text.

  PassageTable           text -> key dictionary over a native table that keeps each distinct passage's WordPiece ids in HBM
  MI355XRerankRetriever  ContextualCompressionRetriever's surface (``base_compressor``, ``base_retriever``, ``invoke``) plus
                         ``compress_documents``, answered by ONE library call: pairs assembled on the device, forward, stable top-n

The retriever returns what ``base_compressor.compress_documents(base_retriever.invoke(query), query)`` returns -- the same documents, order and
``relevance_score`` floats -- and falls back to exactly that call whenever the one call does not serve the request.
"""
from __future__ import annotations

import ctypes
import threading
from typing import Any, Optional, Sequence

import numpy as np

from . import _native as N
from ._lc import BaseRetriever, Document


class _Generation:
    """One native table and its dictionary.  A table that reached its cap is retired: calls that hold keys of it finish on it, then it is freed."""
    __slots__ = ("h", "keys", "lens", "users", "retired")

    def __init__(self, h):
        self.h, self.keys, self.lens, self.users, self.retired = h, {}, [], 0, False


class PassageTable:
    """Content-addressed cache of passage tokens: ``keys_for(texts, tokenizer)`` numbers distinct texts and appends the tokens of the ones seen
    for the first time to the native table (rmu_passages_set).  It knows nothing of a store's add / delete / compact life cycle: a deleted
    document's entry is merely unused.  At ``max_entries`` the table and the dictionary are cleared and refilled on demand.  One lock covers the
    dictionary and the appends; calls from several threads are safe."""

    def __init__(self, cls_id: int, sep_id: int, pad_id: int, max_len: int = 512, max_entries: int = 4_000_000):
        self._lib = N.lib()
        self._ids = (int(cls_id), int(sep_id), int(pad_id))
        self.max_len = int(max_len)
        self.cap = self.max_len - 3                      # tokens an entry keeps: the most a pair can hold of its second text
        self.max_entries = int(max_entries)
        self.clears = 0
        self._lock = threading.Lock()
        self._gen = self._new_generation()

    @classmethod
    def for_tokenizer(cls, tokenizer, max_len: int = 512, **kw) -> "PassageTable":
        """The special ids are the tokenizer's own: what it writes around and behind an empty text."""
        ids, _, lens = tokenizer.encode([""], None, max_len=8)
        assert int(lens[0]) == 2
        return cls(int(ids[0, 0]), int(ids[0, 1]), int(ids[0, 2]), max_len=max_len, **kw)

    def _new_generation(self) -> _Generation:
        h = ctypes.c_void_p()
        N.check(self._lib.rmu_passages_create(ctypes.byref(h), *self._ids, self.max_len), "rmu_passages_create")
        return _Generation(h)

    def _release(self, gen: _Generation):
        if gen.h:
            self._lib.rmu_passages_free(gen.h)
            gen.h = None

    def close(self):
        with self._lock:
            gen = self._gen
            gen.retired = True
            if gen.users == 0:
                self._release(gen)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __len__(self) -> int:
        return len(self._gen.keys)

    def size(self) -> tuple[int, int]:
        """(entries, tokens kept) of the native table."""
        n, t = ctypes.c_int64(), ctypes.c_int64()
        with self._lock:
            N.check(self._lib.rmu_passages_size(self._gen.h, ctypes.byref(n), ctypes.byref(t)), "rmu_passages_size")
        return n.value, t.value

    # ---- keys ---------------------------------------------------------------------------------------------------------------------------------
    def _checkout(self, texts: Sequence[str], tokenizer):
        """-> (generation, keys [n] int64, kept lengths [n]); the generation stays alive until `_checkin`."""
        with self._lock:
            gen = self._gen
            fresh = [t for t in dict.fromkeys(texts) if t not in gen.keys]
            if fresh and gen.keys and len(gen.keys) + len(fresh) > self.max_entries:
                gen.retired = True
                if gen.users == 0:
                    self._release(gen)
                gen = self._gen = self._new_generation()
                self.clears += 1
                fresh = list(dict.fromkeys(texts))
            if fresh:
                ids, _, lens = tokenizer.encode(fresh, None, max_len=self.cap + 2)       # single mode: [CLS] <= cap tokens [SEP]
                kept = (np.asarray(lens, dtype=np.int64) - 2).clip(0, self.cap)
                offsets = np.zeros(len(fresh) + 1, dtype=np.int64)
                np.cumsum(kept, out=offsets[1:])
                mask = np.arange(ids.shape[1] - 1)[None, :] < kept[:, None]
                tokens = np.ascontiguousarray(ids[:, 1:][mask], dtype=np.int32)
                first = len(gen.lens)
                N.check(self._lib.rmu_passages_set(gen.h, first, tokens.ctypes.data, offsets.ctypes.data, len(fresh)), "rmu_passages_set")
                for i, t in enumerate(fresh):
                    gen.keys[t] = first + i
                gen.lens.extend(int(v) for v in kept)
            keys = np.fromiter((gen.keys[t] for t in texts), dtype=np.int64, count=len(texts))
            plens = np.fromiter((gen.lens[k] for k in keys), dtype=np.int64, count=len(texts))
            gen.users += 1
            return gen, keys, plens

    def _checkin(self, gen: _Generation):
        with self._lock:
            gen.users -= 1
            if gen.retired and gen.users == 0:
                self._release(gen)

    def keys_for(self, texts: Sequence[str], tokenizer) -> np.ndarray:
        """The key of each text; equal texts share a key.  Texts seen for the first time are tokenised in ONE tokenizer call and appended."""
        gen, keys, _ = self._checkout(list(texts), tokenizer)
        self._checkin(gen)
        return keys

    def warm(self, texts: Sequence[str], tokenizer) -> None:
        """Preload entries, e.g. right after ``add_documents``: the first rerank that retrieves them then tokenises nothing."""
        self.keys_for(texts, tokenizer)


class MI355XRerankRetriever(BaseRetriever):
    """``ContextualCompressionRetriever(base_compressor=ScoredCrossEncoderReranker(...), base_retriever=...)`` with the rerank answered by one
    library call per request (``MI355XCrossEncoder.rerank``).  ``compress_documents(documents, query)`` has the compressor's contract, so
    ``provenance.compute_rerank_provenance`` takes this object in place of the compressor.  Whenever the one call does not serve a request
    (a sigmoid model, another tokenizer, more than 256 documents, an empty list, ...) the compressor's own ``compress_documents`` answers."""

    base_compressor: Any
    base_retriever: Any

    class Config:
        arbitrary_types_allowed = True

    def compress_documents(self, documents: Sequence[Document], query: str, callbacks: Any = None) -> Sequence[Document]:
        comp = self.base_compressor
        docs = list(documents)
        rerank = getattr(getattr(comp, "model", None), "rerank", None)
        res = rerank(query, [d.page_content for d in docs], comp.top_n) if docs and callable(rerank) else None
        if res is None:
            return comp.compress_documents(documents, query, callbacks)
        return [docs[i].copy(update={"metadata": {**docs[i].metadata, "relevance_score": s}}) for i, s in zip(*res)]

    def _get_relevant_documents(self, query: str, *, run_manager: Any = None, **kw) -> list[Document]:
        return list(self.compress_documents(self.base_retriever.invoke(query), query))

    def batch_invoke(self, queries: list[str]) -> list[list[Document]]:
        """The base retriever's batch (one fused retrieval when it has one), then one rerank call per query: each forward runs at the shape the
        compressor's own call would run at, which is what keeps the scores its scores."""
        queries = list(queries)
        base = self.base_retriever
        lists = base.batch_invoke(queries) if hasattr(base, "batch_invoke") else [base.invoke(q) for q in queries]
        return [list(self.compress_documents(docs, q)) for docs, q in zip(lists, queries)]
