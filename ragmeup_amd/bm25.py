"""BM25 on the device: the sparse member of the reference's retrieval ensemble.

The reference builds ``BM25Retriever.from_texts(...)`` (langchain-community over rank_bm25: a Python loop over every document per
query token, an argsort of all N scores, rebuilt from scratch after every upload -- server/RAGHelper.py:436-443, :492-505, :529-531) and
fuses it with the dense retriever.  ``BM25Index`` is the handle on librmu's inverted index in HBM (include/rmu.h, bm25.hip);
``MI355XBM25Retriever`` carries langchain's BM25Retriever surface over it, plus incremental ``add_documents`` / ``add_texts`` and
``batch_invoke`` (one search for a batch, which ``MI355XEnsembleRetriever.batch_invoke`` looks for).

What the dense store next to it has, it has too: ``delete(ids= / expr= / filter=)`` (the server's /delete handler calls it where the
reference rebuilds the retriever over every remaining text), ``compact()`` / ``compact_threshold``, ``persist(path)`` / ``load(path)`` and
``search_kwargs={"filter": ..., "expr": ...}`` on every ``invoke`` -- so both members of one ensemble keep holding the same records.  After a
removal every score is rank_bm25's over the LIVE documents (N, df, the vocabulary and avgdl are theirs); a filter restricts the candidates
and leaves those statistics alone, as a Milvus or ParadeDB filter does.

Scores are rank_bm25.BM25Okapi's.  Ties: score descending, then the LOWER document id -- rank_bm25's ``argsort()[::-1]`` puts the higher
id first among equal scores and is not stable.  Not provided: upsert by id, the ParadeDB SQL retriever.
"""
from __future__ import annotations

import ctypes
import json
import os
import threading
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

    @classmethod
    def load(cls, path: str) -> "BM25Index":
        """Re-open what ``save`` wrote (host only; removed documents stay removed, options are the defaults)."""
        self = cls.__new__(cls)
        self._lib = N.lib()
        h = ctypes.c_void_p()
        N.check(self._lib.rmu_bm25_load(ctypes.byref(h), os.fsencode(path)), "rmu_bm25_load")
        self._h = h
        return self

    def save(self, path: str):
        N.check(self._lib.rmu_bm25_save(self._h, os.fsencode(path)), "rmu_bm25_save")

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
        """Append documents (host only; the next search uploads their postings and splices them into the image); returns the id of
        the first one."""
        texts = list(texts)
        blob = _blob(texts)
        first = ctypes.c_int64()
        N.check(self._lib.rmu_bm25_add_texts(self._h, blob, len(blob), len(texts), ctypes.byref(first)), "rmu_bm25_add_texts")
        return int(first.value)

    def stat(self) -> dict:
        """docs (ids handed out), vocab, nnz and avgdl of the live corpus -- and, once a document has been removed and until the next
        compact, "live": the number of live documents (while every document is live it equals "docs" and is left out, so a fresh index
        reports the four keys it always did; ``live`` below is there in every state)."""
        out = {}
        for name, what in (("docs", N.BM25_STAT_DOCS), ("vocab", N.BM25_STAT_VOCAB), ("nnz", N.BM25_STAT_NNZ), ("avgdl", N.BM25_STAT_AVGDL),
                           ("live", N.BM25_STAT_LIVE_DOCS)):
            v = ctypes.c_double()
            N.check(self._lib.rmu_bm25_stat(self._h, what, ctypes.byref(v)), "rmu_bm25_stat")
            out[name] = float(v.value) if name == "avgdl" else int(v.value)
        if out["live"] == out["docs"]:
            del out["live"]
        return out

    def image_stat(self) -> dict:
        """What the device image has cost so far: "packs" (whole image packed and uploaded), "splices" (only the added documents'
        postings uploaded and spliced in on the device) and "upload_bytes" (postings and posting pointers sent, both paths); all 0
        until the first search."""
        out = {}
        for name, what in (("packs", N.BM25_STAT_IMAGE_PACKS), ("splices", N.BM25_STAT_IMAGE_SPLICES),
                           ("upload_bytes", N.BM25_STAT_IMAGE_UPLOAD_BYTES)):
            v = ctypes.c_double()
            N.check(self._lib.rmu_bm25_stat(self._h, what, ctypes.byref(v)), "rmu_bm25_stat")
            out[name] = int(v.value)
        return out

    def __len__(self) -> int:
        return self.stat()["docs"]

    @property
    def live(self) -> int:
        """Live documents: ``len(self)`` minus the removed ones."""
        st = self.stat()
        return st.get("live", st["docs"])

    def df(self, term: str) -> int:
        v = ctypes.c_int64()
        N.check(self._lib.rmu_bm25_df(self._h, term.encode("utf-8", "surrogatepass"), ctypes.byref(v)), "rmu_bm25_df")
        return int(v.value)

    def set_option(self, option: int, value: int):
        N.check(self._lib.rmu_bm25_set_option(self._h, int(option), int(value)), "rmu_bm25_set_option")

    def remove(self, ids) -> int:
        """Remove documents by id (host only; one recount of df per call, so pass the ids together); returns how many were live."""
        ids = np.ascontiguousarray(np.asarray(ids, dtype=np.int64).reshape(-1))
        n = ctypes.c_int64()
        N.check(self._lib.rmu_bm25_remove_docs(self._h, ids.ctypes.data, ids.size, ctypes.byref(n)), "rmu_bm25_remove_docs")
        return int(n.value)

    def compact(self) -> np.ndarray:
        """Reclaim removed documents: live ones become 0 .. live-1 in order.  Returns the map old id -> new id (-1 = removed)."""
        before = len(self)
        m = np.empty(before + 1, np.int64)               # (+ 1: never an empty buffer; the entries past the documents hold -1)
        N.check(self._lib.rmu_bm25_compact(self._h, m.ctypes.data, m.size, None), "rmu_bm25_compact")
        return m[:before]

    def search(self, queries: list[str], k: int, doc_base: int = 0, stream: int = 0, docs=None):
        """(scores [nq, k] float32, docs [nq, k] int64), best first; slots beyond the live corpus hold (-inf, -1).  ``docs``: an ascending
        int64 array of document ids -- the candidates are its live documents, the statistics stay the corpus's (rmu_bm25_search_subset)."""
        queries = list(queries)
        nq = len(queries)
        scores = np.empty((nq, int(k)), np.float32)
        out = np.empty((nq, int(k)), np.int64)
        if nq == 0:
            return scores, out
        blob = _blob(queries)
        if docs is None:
            N.check(self._lib.rmu_bm25_search(self._h, blob, len(blob), nq, int(k), int(doc_base), scores.ctypes.data, out.ctypes.data,
                                              int(stream)), "rmu_bm25_search")
        else:
            docs = np.ascontiguousarray(np.asarray(docs, dtype=np.int64).reshape(-1))
            N.check(self._lib.rmu_bm25_search_subset(self._h, blob, len(blob), nq, int(k), int(doc_base), docs.ctypes.data, docs.size,
                                                     scores.ctypes.data, out.ctypes.data, int(stream)), "rmu_bm25_search_subset")
        return scores, out


def _joined(tokens) -> str:
    """Tokens of a caller's preprocess_func -> the text whose str.split() gives them back."""
    toks = list(tokens)
    for t in toks:
        if not isinstance(t, str) or not t or any(ch.isspace() for ch in t):
            raise ValueError(f"preprocess_func returned {t!r}: every token must be a non-empty string without whitespace")
    return " ".join(toks)


class MI355XBM25Retriever(BaseRetriever):
    """``BM25Retriever`` (langchain-community) over ``BM25Index``: fields ``vectorizer`` (the index), ``docs``, ``k`` and
    ``preprocess_func`` (None = str.split(), langchain's default, done inside the library).  Beside langchain's surface, what
    ``MI355XVectorStore`` offers for the same records: ``delete``, ``compact`` / ``compact_threshold``, ``persist`` / ``load`` and
    ``search_kwargs`` with ``"filter"`` / ``"expr"``.  ``docs[i]`` is the document with id ``i``, removed ones included until ``compact``."""

    vectorizer: Any = None
    docs: List[Any] = []
    k: int = 4
    preprocess_func: Optional[Callable[[str], List[str]]] = None
    search_kwargs: dict = {}
    compact_threshold: Optional[float] = None

    class Config:
        arbitrary_types_allowed = True

    # ---- private records beside `docs`: liveness, the ids given at add time, the cached filter results -----------------------------
    def _st(self) -> dict:
        st = self.__dict__.get("_bm25_state")
        if st is None:
            st = {"alive": [], "ids": [], "rows": {}, "gen": 0, "lock": threading.RLock()}
            object.__setattr__(self, "_bm25_state", st)
        n = len(self.docs)
        if len(st["alive"]) < n:                          # documents handed to the constructor
            st["ids"] += [getattr(d, "id", None) for d in self.docs[len(st["ids"]):n]]
            st["alive"] += [True] * (n - len(st["alive"]))
        return st

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

    @staticmethod
    def _document(text, meta, i) -> Document:
        d = Document(page_content=text, metadata=dict(meta or {}))
        if i is not None:
            try:
                d.id = i
            except (AttributeError, ValueError):   # a Document type without an id
                pass
        return d

    def add_texts(self, texts: Iterable[str], metadatas: Optional[Iterable[dict]] = None, ids: Optional[Iterable[str]] = None) -> list:
        texts = list(texts)
        metadatas = list(metadatas) if metadatas is not None else [{} for _ in texts]
        ids = list(ids) if ids is not None else [None] * len(texts)
        if not (len(texts) == len(metadatas) == len(ids)):
            raise ValueError("texts, metadatas and ids differ in length")
        prepared = [self._text(t) for t in texts]
        st = self._st()
        with st["lock"]:
            first = self.vectorizer.add_texts(prepared)
            assert first == len(self.docs)
            for t, m, i in zip(texts, metadatas, ids):
                self.docs.append(self._document(t, m, i))
            st["ids"] += ids
            st["alive"] += [True] * len(texts)
            st["rows"] = {}
        return ids

    def add_documents(self, documents: Iterable[Document], ids: Optional[Iterable[str]] = None) -> list:
        """Incremental upload (the reference rebuilds the whole retriever instead, RAGHelper.py:529-531)."""
        documents = list(documents)
        return self.add_texts([d.page_content for d in documents], [d.metadata for d in documents],
                              ids if ids is not None else [getattr(d, "id", None) for d in documents])

    # ---- conditions over the records: the store's language (MI355XVectorStore._conditions), evaluated over docs[i].metadata and the id ---
    def _matching(self, conds) -> np.ndarray:
        """Ascending int64 ids of the live documents that satisfy every condition; "pk" names the document's id."""
        st = self._st()
        out = []
        for r, (d, alive, pk) in enumerate(zip(self.docs, st["alive"], st["ids"])):
            if alive and all(any(v == x for x in vals) or v == vals
                             for v, vals in ((pk if f == "pk" else d.metadata.get(f), vals) for f, vals in conds)):
                out.append(r)
        return np.asarray(out, dtype=np.int64)

    def _candidates(self):
        """The document ids search_kwargs' "filter" / "expr" admit (None: no restriction), cached until the records change."""
        from .vectorstore import MI355XVectorStore
        kw = self.search_kwargs or {}
        expr, flt = kw.get("expr"), kw.get("filter")
        if expr is None and flt is None:
            return None
        st = self._st()
        key = repr((expr, flt))
        rows = st["rows"].get(key)
        if rows is None:
            conds = MI355XVectorStore._conditions(expr, flt)
            if conds is None:
                return None
            with st["lock"]:
                rows = self._matching(conds)
                st["rows"] = {key: rows}
        return rows

    def delete(self, ids: Optional[list] = None, expr: Optional[str] = None, filter: Optional[dict] = None, **kw):
        """Delete by document id list, by a Milvus-style expression or by a metadata dict: the three selectors of
        ``MI355XVectorStore.delete``, parsed by the store's own code.  Where the reference's /delete handler (server.py:353-385) calls
        ``loadData()`` to rebuild BM25 without the file, call this.  Returns the store's result type (``delete_count``)."""
        from .vectorstore import MI355XVectorStore, _DeleteResult
        st = self._st()
        with st["lock"]:
            rows: list[int] = []
            if ids:
                want = set(ids)
                rows += [r for r, pk in enumerate(st["ids"]) if pk is not None and pk in want]
            conds = MI355XVectorStore._conditions(expr or None, filter or None)
            if conds:
                rows += self._matching(conds).tolist()
            rows = sorted({r for r in rows if st["alive"][r]})
            if rows:
                n = self.vectorizer.remove(rows)
                assert n == len(rows)
                for r in rows:
                    st["alive"][r] = False
                st["rows"] = {}
                thr = self.compact_threshold
                if thr is not None and len(st["alive"]) - sum(st["alive"]) > float(thr) * len(st["alive"]):
                    self.compact()
        return _DeleteResult(len(rows))

    def compact(self) -> int:
        """Reclaim the removed documents in the index and renumber ``docs`` with its map; returns how many were reclaimed."""
        st = self._st()
        with st["lock"]:
            if all(st["alive"]):
                return 0
            before = len(self.docs)
            st["gen"] += 1                                # odd: a search that overlaps this section repeats
            try:
                keep = np.flatnonzero(self.vectorizer.compact() >= 0).tolist()
                docs, pks = self.docs, st["ids"]
                self.docs = [docs[r] for r in keep]
                st["ids"] = [pks[r] for r in keep]
                st["alive"] = [True] * len(keep)
                st["rows"] = {}
            finally:
                st["gen"] += 1
            return before - len(keep)

    # ---- persistence: the index file + one JSON record per document ---------------------------------------------------------------------
    def persist(self, path: str):
        """Write ``path + ".bm25"`` (rmu_bm25_save) and ``path + ".docs.jsonl"`` (text, metadata, id, alive per line)."""
        from .vectorstore import _json_default
        st = self._st()
        with st["lock"]:
            self.vectorizer.save(path + ".bm25")
            with open(path + ".docs.jsonl", "w", encoding="utf-8") as f:
                for d, alive, pk in zip(self.docs, st["alive"], st["ids"]):
                    f.write(json.dumps({"text": d.page_content, "metadata": d.metadata, "id": pk, "alive": 1 if alive else 0},
                                       default=_json_default) + "\n")

    @classmethod
    def load(cls, path: str, preprocess_func: Optional[Callable[[str], List[str]]] = None, **kwargs: Any):
        """Re-open what ``persist`` wrote: no text is tokenised again.  ``preprocess_func`` must be the one the index was built with."""
        with open(path + ".docs.jsonl", encoding="utf-8") as f:
            recs = [json.loads(line) for line in f if line.strip()]
        ix = BM25Index.load(path + ".bm25")
        if len(ix) != len(recs) or ix.live != sum(1 for r in recs if r["alive"]):
            ix.close()
            raise ValueError(f"{path}: the index file and the document records are out of step")
        self = cls(vectorizer=ix, docs=[cls._document(r["text"], r["metadata"], r["id"]) for r in recs], preprocess_func=preprocess_func,
                   **kwargs)
        st = self._st()
        st["ids"] = [r["id"] for r in recs]
        st["alive"] = [bool(r["alive"]) for r in recs]
        return self

    def batch_invoke(self, queries: list[str]) -> list[list[Document]]:
        """One rmu_bm25_search for the whole batch (rmu_bm25_search_subset under a filter); a removed document never comes back."""
        queries = list(queries)
        if not queries or not self.docs:
            return [[] for _ in queries]
        st = self._st()
        texts = [self._text(q) for q in queries]
        while True:
            g = st["gen"]
            if g & 1:                                     # a compaction is renumbering: it holds the lock until it is done
                with st["lock"]:
                    pass
                continue
            docs = self.docs
            try:
                _, rows = self.vectorizer.search(texts, min(int(self.k), N.MAX_K), docs=self._candidates())
                out = [[docs[r] for r in row if r >= 0] for row in rows.tolist()]
            except Exception:
                if st["gen"] != g:                        # e.g. an id that no longer exists
                    continue
                raise
            if st["gen"] == g:
                return out

    def _get_relevant_documents(self, query: str, *, run_manager: Any = None, **kw) -> list[Document]:
        return self.batch_invoke([query])[0]
