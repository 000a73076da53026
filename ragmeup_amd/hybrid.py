"""The ensemble's retrieval step in one library call: BM25 top-k, dense top-fetch_k + MMR and their weighted reciprocal-rank fusion on the
device, one synchronisation (include/rmu.h, "hybrid retrieval"; rrf_fuse.hip).

The reference answers every request through ``EnsembleRetriever([bm25, dense_mmr], weights=[0.5, 0.5])`` (server/RAGHelper.py:497-503,
RAGHelper_local.py:251-259).  ``MI355XEnsembleRetriever`` (ensemble.py) is that fusion as host code over two member calls, each with its own
synchronisation and copy; ``MI355XHybridRetriever`` has the same surface (``invoke``, ``batch_invoke``) and returns the same documents in the
same order, from ``rmu_hybrid_search`` / ``rmu_bert_search_hybrid``.  ``HybridIndex`` is the ctypes handle.

Documents are identified by ``page_content``, as langchain's fusion does: ``content_keys`` numbers the distinct texts in first-seen order and
the library fuses those numbers.  The retriever keeps one key per BM25 document id and one per store row and refreshes a member's table when
that member's records changed behind its back (an upload, a delete + compact, a rebuilt BM25 retriever): detection, not ownership of the add
path, because the reference's server changes the members directly.

Whatever the one call cannot serve -- a ``filter`` / ``expr`` on either member, per-request ``filters=`` / ``exprs=`` of ``batch_invoke``, ``fetch_k`` > 64, a dense ``search_type`` other than
``similarity`` / ``mmr``, a caller ``preprocess_func``, a pending pipelined insert -- takes the two member calls and
``weighted_reciprocal_rank``: the same result by definition.
"""
from __future__ import annotations

import ctypes
import threading
from typing import Any, Iterable, List, Optional

import numpy as np

from . import _native as N
from ._lc import BaseRetriever, Document
from .bm25 import BM25Index, MI355XBM25Retriever, _blob
from .ensemble import per_query_conditions, weighted_reciprocal_rank
from .records import consistent
from .vectorstore import MI355XRetriever, MI355XVectorStore


def content_keys(texts: Iterable[str], classes: dict) -> np.ndarray:
    """int64 key of every text: equal texts share a key, keys are handed out in first-seen order.  ``classes`` (text -> key) carries the
    numbering from call to call, so both members of one retriever draw from the same classes."""
    out = []
    for t in texts:
        k = classes.get(t)
        if k is None:
            k = classes[t] = len(classes)
        out.append(k)
    return np.asarray(out, dtype=np.int64)


class HybridIndex:
    """``rmu_hybrid_*``: the two members behind one handle, their key tables, and the one-call search.  The members (a ``BM25Index`` and a
    ``FlatIndex``, either may be None) are borrowed: this object keeps them referenced, and must not be searched after one was closed."""

    def __init__(self, sparse: Optional[BM25Index], dense: Any):
        self._lib = N.lib()
        self.sparse, self.dense = sparse, dense
        h = ctypes.c_void_p()
        N.check(self._lib.rmu_hybrid_create(ctypes.byref(h), sparse._h if sparse is not None else None, dense._h if dense is not None else None),
                "rmu_hybrid_create")
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            self._lib.rmu_hybrid_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_keys(self, member: int, first: int, keys):
        """Write keys[0:n] to entries [first, first + n) of ``member``'s table (0 = sparse, 1 = dense); the table ends there afterwards."""
        keys = np.ascontiguousarray(np.asarray(keys, dtype=np.int64).reshape(-1))
        N.check(self._lib.rmu_hybrid_set_keys(self._h, int(member), int(first), keys.ctypes.data if keys.size else None, keys.size),
                "rmu_hybrid_set_keys")

    @staticmethod
    def _outputs(nq: int, k_out: int):
        return np.empty((nq, k_out), np.float64), np.empty((nq, k_out), np.int64), np.empty((nq, k_out), np.int32)

    @staticmethod
    def _weights(weights):
        w = (ctypes.c_double * 2)(float(weights[0]), float(weights[1]))
        return w

    def search(self, q, queries: list[str], k_sparse: int, fetch_k: int, k_dense: int, lambda_mult: Optional[float] = 0.5,
               weights=(0.5, 0.5), c: int = 60, k_out: Optional[int] = None, stream: int = 0):
        """(scores [nq, k_out] float64, ids [nq, k_out] int64, member [nq, k_out] int32): the fused hits of ``queries`` (text, for the
        sparse member) and ``q`` ([nq, dim] float32, the same queries embedded); each hit is named by the member that represents it and
        that member's own id; slots past the distinct hits hold (-inf, -1, -1).  ``lambda_mult`` None: no MMR selection."""
        queries = list(queries)
        nq = len(queries)
        k_out = int(k_sparse) + int(k_dense) if k_out is None else int(k_out)
        q = np.ascontiguousarray(np.asarray(q, dtype=np.float32).reshape(nq, -1))
        scores, ids, member = self._outputs(nq, k_out)
        blob = _blob(queries)
        N.check(self._lib.rmu_hybrid_search(self._h, q.ctypes.data, nq, blob, len(blob), int(k_sparse), int(fetch_k), int(k_dense),
                                            -1.0 if lambda_mult is None else float(lambda_mult), self._weights(weights), int(c), k_out,
                                            scores.ctypes.data, ids.ctypes.data, member.ctypes.data, int(stream)), "rmu_hybrid_search")
        return scores, ids, member

    def search_tokens(self, encoder, tok_ids, lens, mode: int, queries: list[str], k_sparse: int, fetch_k: int, k_dense: int,
                      lambda_mult: Optional[float] = 0.5, weights=(0.5, 0.5), c: int = 60, k_out: Optional[int] = None):
        """``search`` behind the native encoder's forward (rmu_bert_search_hybrid): the queries' token ids in, the pooled vectors never
        leave the device.  The batch is padded to the encoder's bucketed shape with empty queries, whose rows are dropped."""
        queries = list(queries)
        pi, pl, _, B, bb, lb = encoder._host_arrays(tok_ids, lens, None, mode)
        assert B == len(queries)
        k_out = int(k_sparse) + int(k_dense) if k_out is None else int(k_out)
        scores, ids, member = self._outputs(bb, k_out)
        blob = _blob(queries + [""] * (bb - B))
        N.check(self._lib.rmu_bert_search_hybrid(encoder._h, self._h, pi.ctypes.data, None, pl.ctypes.data, int(bb), int(lb), int(mode), blob,
                                                 len(blob), int(k_sparse), int(fetch_k), int(k_dense),
                                                 -1.0 if lambda_mult is None else float(lambda_mult), self._weights(weights), int(c), k_out,
                                                 scores.ctypes.data, ids.ctypes.data, member.ctypes.data), "rmu_bert_search_hybrid")
        return scores[:B], ids[:B], member[:B]


class MI355XHybridRetriever(BaseRetriever):
    """``EnsembleRetriever(retrievers=[sparse, dense], weights=[...])`` over an ``MI355XBM25Retriever`` and the ``MI355XRetriever`` of
    ``store.as_retriever(...)``, answered by one library call per ``invoke`` / ``batch_invoke``.  Same documents, same order as
    ``MI355XEnsembleRetriever(retrievers=[sparse, dense], weights=weights, c=c)``."""

    sparse: Any
    dense: Any
    weights: List[float] = []
    c: int = 60

    class Config:
        arbitrary_types_allowed = True

    _MAX_OUT_OF_STEP = 8      # a member changed between the table refresh and the search: refresh again, this often at most

    def _weights(self) -> list[float]:
        return list(self.weights) if self.weights else [0.5, 0.5]

    # ---- private state: the handle, the classes of page_content, one stamp per member ------------------------------------------------
    def _st(self) -> dict:
        st = self.__dict__.get("_hybrid_state")
        if st is None:
            st = {"handle": None, "members": None, "classes": {}, "stamp": [None, None], "lock": threading.RLock()}
            object.__setattr__(self, "_hybrid_state", st)
        return st

    def close(self):
        st = self._st()
        with st["lock"]:
            if st["handle"] is not None:
                st["handle"].close()
            st["handle"], st["members"], st["stamp"] = None, None, [None, None]

    def _plan(self):
        """(k_sparse, fetch_k, k_dense, lambda_mult) when the one call serves this configuration, else None (the two-call fusion)."""
        sp, de = self.sparse, self.dense
        if not isinstance(sp, MI355XBM25Retriever) or not isinstance(de, MI355XRetriever):
            return None
        store = de.vectorstore
        if not isinstance(store, MI355XVectorStore) or not isinstance(sp.vectorizer, BM25Index):
            return None
        skw = sp.search_kwargs or {}
        if sp.preprocess_func is not None or skw.get("filter") is not None or skw.get("expr") is not None:
            return None
        kw = dict(de.search_kwargs or {})
        if store._pending or store._index is None or not getattr(store._index, "_h", None) or not getattr(sp.vectorizer, "_h", None):
            return None
        k_sparse = min(int(sp.k), N.MAX_K)
        k = int(kw.get("k", 4))
        if de.search_type == "mmr":
            if set(kw) - {"k", "fetch_k", "lambda_mult"}:
                return None
            fetch_k, lam = int(kw.get("fetch_k", 20)), float(kw.get("lambda_mult", 0.5))
            if lam < 0.0:
                return None
        elif de.search_type == "similarity":
            if set(kw) - {"k"}:
                return None
            fetch_k, lam = k, None
        else:
            return None
        if k_sparse < 1 or not (1 <= k <= fetch_k <= 64):
            return None
        return k_sparse, fetch_k, k, lam

    def _sync(self, st) -> tuple:
        """(under st["lock"]) the handle over the members' current indexes, its tables brought in step with the members' records; returns
        (handle, the sparse member's documents as the table saw them)."""
        sp, store = self.sparse, self.dense.vectorstore
        members = (sp.vectorizer, store._index)
        if st["handle"] is None or st["members"][0] is not members[0] or st["members"][1] is not members[1]:
            if st["handle"] is not None:
                st["handle"].close()
            st["handle"], st["members"], st["stamp"] = HybridIndex(*members), members, [None, None]
        h = st["handle"]
        docs, texts = sp.docs, store._texts
        stamps = ((id(sp), len(docs), sp._st()["seq"].value), (id(store), len(texts), store._seq.value))
        for m, (records, stamp) in enumerate(zip((docs, texts), stamps)):
            old = st["stamp"][m]
            if old == stamp:
                continue
            # the same records with more behind them: an append.  Anything else (a compaction, another retriever / store): a replacement
            first = old[1] if old is not None and old[0] == stamp[0] and old[2] == stamp[2] and old[1] <= stamp[1] else 0
            new = records[first:stamp[1]]
            h.set_keys(m, first, content_keys((d.page_content for d in new) if m == 0 else new, st["classes"]))
            st["stamp"][m] = stamp
        return h, docs

    def _one_call(self, queries: list[str], plan, single: bool):
        sp, store = self.sparse, self.dense.vectorstore
        k_sparse, fetch_k, k_dense, lam = plan
        st = self._st()
        emb = store._embeddings
        # the query vectors, as the dense member's own invoke / batch_invoke makes them
        tokens = vecs = None
        if single and hasattr(emb, "query_ids") and getattr(store._index, "dim", 0) == 384:
            tokens = emb.query_ids(queries[0])
        if tokens is None:
            vecs = store._embed_query(queries[0])[None] if single else store._embed_docs(queries)

        def search():
            with st["lock"]:
                h, docs = self._sync(st)
            if tokens is not None:
                _, ids, member = h.search_tokens(emb.encoder, tokens[0], tokens[1], emb._mode, queries, k_sparse, fetch_k, k_dense, lam,
                                                 self._weights(), self.c)
            else:
                _, ids, member = h.search(vecs, queries, k_sparse, fetch_k, k_dense, lam, self._weights(), self.c)
            return [[docs[i] if m == 0 else store._doc(i) for i, m in zip(row_i, row_m) if i >= 0]
                    for row_i, row_m in zip(ids.tolist(), member.tolist())]

        def read():
            for tries in range(self._MAX_OUT_OF_STEP + 1):
                try:
                    return search()
                except N.RmuError as e:                       # records were added between the refresh and the search: refresh again
                    if "out of step" not in str(e) or tries == self._MAX_OUT_OF_STEP:
                        raise
        # (a compaction of either member renumbers what the tables name: the read is repeated)
        return consistent(read, sp._st()["seq"], store._seq)

    def batch_invoke(self, queries: list[str], filters: Optional[list] = None, exprs: Optional[list] = None) -> list[list[Document]]:
        """`filters` / `exprs`: one condition per query (None = unfiltered).  The one call takes no lists, so a per-request form takes
        the two member batch calls (each one grouped call) and the host fusion: the route a `search_kwargs` filter takes."""
        queries = list(queries)
        each = per_query_conditions([self.sparse, self.dense], filters, exprs)
        if not queries:
            return []
        plan = None if each else self._plan()
        if plan is None:
            per = [self.sparse.batch_invoke(queries, **each), self.dense.batch_invoke(queries, **each)]
            return [weighted_reciprocal_rank([m[i] for m in per], self._weights(), self.c) for i in range(len(queries))]
        return self._one_call(queries, plan, single=False)

    def _get_relevant_documents(self, query: str, *, run_manager: Any = None, **kw) -> list[Document]:
        plan = self._plan()
        if plan is None:
            return weighted_reciprocal_rank([self.sparse.invoke(query), self.dense.invoke(query)], self._weights(), self.c)
        return self._one_call([query], plan, single=True)[0]
