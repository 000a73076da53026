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
``batch_invoke(queries, exprs=[...])`` (or ``filters=[...]``) gives every request its own condition; the distinct lists share one
``rmu_bm25_search_groups`` launch whose work follows the lists (profiles/bm25_groups.md).

Scores are rank_bm25.BM25Okapi's.  Ties: score descending, then the LOWER document id -- rank_bm25's ``argsort()[::-1]`` puts the higher
id first among equal scores and is not stable.  Not provided: upsert by id, the ParadeDB SQL retriever.
"""
from __future__ import annotations

import ctypes
import json
import os
import threading
from typing import Any, Callable, ClassVar, Iterable, List, Optional

import numpy as np

from . import _native as N
from ._lc import BaseRetriever, Document
from .records import (DeleteResult, FieldMaps, Seqlock, conditions, conditions_per_query, consistent, flatten_groups, group_conditions,
                      json_default)


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

    MAX_QUERIES_PER_CALL = 65535     # rmu_bm25_search's limit on nq

    def search_groups(self, queries: list[str], k: int, lists, q_list, doc_base: int = 0, stream: int = 0):
        """Top-k of every query among ITS OWN list of documents, all in one launch (rmu_bm25_search_groups): ``lists`` is a sequence of
        strictly ascending int64 id arrays (they may overlap, repeat each other, be empty or go unused), ``q_list[i]`` the list of query
        i, in any order.  numpy in -> numpy out: for query i exactly what ``search([queries[i]], k, docs=lists[q_list[i]])`` returns,
        bit for bit.  The queries are sorted by list (stably), only the lists a call uses are sent, and the results are put back in the
        caller's order."""
        from .index import search_groups_blocks
        texts = np.empty(len(queries), dtype=object)
        texts[:] = list(queries)

        def call(q_block, kk, docs, list_ptr, ql, base):
            return self._groups_call(list(q_block), kk, docs, list_ptr, ql, base, int(stream))

        return search_groups_blocks(call, texts, int(k), lists, q_list, int(doc_base), block=self.MAX_QUERIES_PER_CALL)

    def _groups_call(self, queries: list[str], k: int, docs: np.ndarray, list_ptr: np.ndarray, q_list: np.ndarray, doc_base: int, stream: int):
        """One rmu_bm25_search_groups call: docs = the lists end to end (int64), list_ptr int64 [n_lists + 1], q_list int32 [nq]
        non-decreasing."""
        nq = len(queries)
        scores = np.empty((nq, k), np.float32)
        out = np.empty((nq, k), np.int64)
        blob = _blob(queries)
        N.check(self._lib.rmu_bm25_search_groups(self._h, blob, len(blob), nq, k, doc_base, docs.ctypes.data, list_ptr.ctypes.data,
                                                 int(list_ptr.shape[0]) - 1, q_list.ctypes.data, scores.ctypes.data, out.ctypes.data, stream),
                "rmu_bm25_search_groups")
        return scores, out


def _joined(tokens) -> str:
    """Tokens of a caller's preprocess_func -> the text whose str.split() gives them back."""
    toks = list(tokens)
    for t in toks:
        if not isinstance(t, str) or not t or any(ch.isspace() for ch in t):
            raise ValueError(f"preprocess_func returned {t!r}: every token must be a non-empty string without whitespace")
    return " ".join(toks)


def _records_changed(st: dict):
    """(under the retriever's lock) documents were added, removed or renumbered: the cached id list and the field maps no longer hold"""
    st["rows"] = {}
    st["fields"].changed()


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

    # ---- private records beside `docs`: liveness, the ids given at add time, the cached filter result, the field maps over all three
    # ("fields"; _matching hands them the three sequences) and the seqlock of compact() ("seq", whose
    # lock is the writer lock) -----------------------------------------------------------------------------------------------------------
    def _st(self) -> dict:
        st = self.__dict__.get("_bm25_state")
        if st is None:
            lock = threading.RLock()
            st = {"alive": [], "ids": [], "rows": {}}
            st["fields"] = FieldMaps(lock)
            st["seq"] = Seqlock(lock, lambda: _records_changed(st))
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
        with st["seq"].lock:
            first = self.vectorizer.add_texts(prepared)
            assert first == len(self.docs)
            for t, m, i in zip(texts, metadatas, ids):
                self.docs.append(self._document(t, m, i))
            st["ids"] += ids
            st["alive"] += [True] * len(texts)
            _records_changed(st)
        return ids

    def add_documents(self, documents: Iterable[Document], ids: Optional[Iterable[str]] = None) -> list:
        """Incremental upload (the reference rebuilds the whole retriever instead, RAGHelper.py:529-531)."""
        documents = list(documents)
        return self.add_texts([d.page_content for d in documents], [d.metadata for d in documents],
                              ids if ids is not None else [getattr(d, "id", None) for d in documents])

    # ---- conditions over the records: the store's language (records.conditions), evaluated over docs[i].metadata and the id ------------
    def _matching(self, conds) -> np.ndarray:
        """Ascending int64 ids of the live documents that satisfy every condition; "pk" names the document's id."""
        st = self._st()
        return st["fields"].matching(conds, lambda: (st["alive"], st["ids"], [d.metadata for d in self.docs]))

    def _candidates(self):
        """The document ids search_kwargs' "filter" / "expr" admit (None: no restriction), cached until the records change."""
        kw = self.search_kwargs or {}
        expr, flt = kw.get("expr"), kw.get("filter")
        if expr is None and flt is None:
            return None
        st = self._st()
        key = repr((expr, flt))
        rows = st["rows"].get(key)
        if rows is None:
            conds = conditions(expr, flt)
            if conds is None:
                return None
            with st["seq"].lock:
                rows = self._matching(conds)
                st["rows"] = {key: rows}
        return rows

    def delete(self, ids: Optional[list] = None, expr: Optional[str] = None, filter: Optional[dict] = None, **kw):
        """Delete by document id list, by a Milvus-style expression or by a metadata dict: the three selectors of
        ``MI355XVectorStore.delete``, parsed by the store's own code.  Where the reference's /delete handler (server.py:353-385) calls
        ``loadData()`` to rebuild BM25 without the file, call this.  Returns the store's result type (``delete_count``)."""
        st = self._st()
        with st["seq"].lock:
            rows: list[int] = []
            if ids:
                want = set(ids)
                rows += [r for r, pk in enumerate(st["ids"]) if pk is not None and pk in want]
            conds = conditions(expr or None, filter or None)
            if conds:
                rows += self._matching(conds).tolist()
            rows = sorted({r for r in rows if st["alive"][r]})
            if rows:
                n = self.vectorizer.remove(rows)
                assert n == len(rows)
                for r in rows:
                    st["alive"][r] = False
                _records_changed(st)
                thr = self.compact_threshold
                if thr is not None and len(st["alive"]) - sum(st["alive"]) > float(thr) * len(st["alive"]):
                    self.compact()
        return DeleteResult(len(rows))

    def compact(self) -> int:
        """Reclaim the removed documents in the index and renumber ``docs`` with its map; returns how many were reclaimed."""
        st = self._st()
        with st["seq"].lock:
            if all(st["alive"]):
                return 0
            before = len(self.docs)
            with st["seq"].write():                       # (a search that overlaps this section repeats; the caches are dropped on the way out)
                keep = np.flatnonzero(self.vectorizer.compact() >= 0).tolist()
                docs, pks = self.docs, st["ids"]
                self.docs = [docs[r] for r in keep]
                st["ids"] = [pks[r] for r in keep]
                st["alive"] = [True] * len(keep)
            return before - len(keep)

    # ---- persistence: the index file + one JSON record per document ---------------------------------------------------------------------
    def persist(self, path: str):
        """Write ``path + ".bm25"`` (rmu_bm25_save) and ``path + ".docs.jsonl"`` (text, metadata, id, alive per line)."""
        st = self._st()
        with st["seq"].lock:
            self.vectorizer.save(path + ".bm25")
            with open(path + ".docs.jsonl", "w", encoding="utf-8") as f:
                for d, alive, pk in zip(self.docs, st["alive"], st["ids"]):
                    f.write(json.dumps({"text": d.page_content, "metadata": d.metadata, "id": pk, "alive": 1 if alive else 0},
                                       default=json_default) + "\n")

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
        _records_changed(st)
        return self

    # The grouped call (BM25Index.search_groups) answers two or more distinct lists in one launch.  profiles/bm25_groups.md measures it
    # against the per-list subset calls it replaces (1M documents, k = 4, lists of contiguous and of random ids, 1 and 4 queries per list).
    # Each row: (documents in the longest list at most, distinct lists at least, at most) -- exactly where the table has the grouped call
    # ahead by more than the run-to-run spread in every run.  Not decided there, so the per-list loop stays: 2 lists of 10 000 documents
    # (random ids: 0.88x and 1.04x), 2 and 128 lists of 100 000.  Not measured: more than 128 lists, lists beyond 100 000 documents.
    GROUPS_RULE: ClassVar[tuple] = ((1_000, 2, 128), (10_000, 8, 128), (100_000, 8, 32))

    @classmethod
    def _use_groups(cls, index, lists: list) -> bool:
        if len(lists) < 2 or not hasattr(index, "search_groups"):
            return False
        longest = max(int(l.size) for l in lists)
        for docs_at_most, lists_at_least, lists_at_most in cls.GROUPS_RULE:
            if longest <= docs_at_most:
                return lists_at_least <= len(lists) <= lists_at_most
        return False

    def _search_each(self, texts: list[str], k: int, conds_each: list) -> np.ndarray:
        """One condition per query (None = unfiltered), inside batch_invoke's consistent read: equal conditions share one list, the unfiltered
        queries take the ordinary search, one distinct list takes the subset call, two or more take the grouped call where
        profiles/bm25_groups.md has it ahead, an empty selection costs no launch.  -> ids [nq, k], padded with -1."""
        nq = len(texts)
        rows = np.full((nq, k), -1, np.int64)
        plain, conds, q_of = group_conditions(conds_each)
        if plain:
            rows[plain] = self.vectorizer.search([texts[i] for i in plain], k)[1]
        lists = [self._matching(c) for c in conds]
        used = [g for g in range(len(lists)) if lists[g].size]      # (an empty selection: its queries keep the padding)
        if self._use_groups(self.vectorizer, [lists[g] for g in used]):
            qi, ql = flatten_groups([q_of[g] for g in used])
            rows[qi] = self.vectorizer.search_groups([texts[i] for i in qi], k, [lists[g] for g in used], ql)[1]
        else:
            for g in used:
                rows[q_of[g]] = self.vectorizer.search([texts[i] for i in q_of[g]], k, docs=lists[g])[1]
        return rows

    def batch_invoke(self, queries: list[str], filters: Optional[list] = None, exprs: Optional[list] = None) -> list[list[Document]]:
        """One rmu_bm25_search for the whole batch (rmu_bm25_search_subset under a filter); a removed document never comes back.
        ``filters`` / ``exprs``: one condition per query (None = unfiltered), e.g. every request asking about its own upload -- the
        conditions are resolved through the cached field maps and the distinct lists share one rmu_bm25_search_groups call."""
        queries = list(queries)
        kw = self.search_kwargs or {}
        each = conditions_per_query(len(queries), kw.get("expr"), kw.get("filter"), exprs, filters)
        if not queries or not self.docs:
            return [[] for _ in queries]
        texts = [self._text(q) for q in queries]

        def read():
            docs = self.docs
            k = min(int(self.k), N.MAX_K)
            if each is None:
                _, rows = self.vectorizer.search(texts, k, docs=self._candidates())
            else:                                         # (resolved here: a compaction cannot slip between the lists and the search)
                rows = self._search_each(texts, k, each)
            return [[docs[r] for r in row if r >= 0] for row in rows.tolist()]
        return consistent(read, self._st()["seq"])

    def _get_relevant_documents(self, query: str, *, run_manager: Any = None, **kw) -> list[Document]:
        return self.batch_invoke([query])[0]
