"""Similarity provenance -- the reference's ``DocumentSimilarityAttribution`` (server/provenance.py:164-202, ``provenance_method=similarity``;
called once per /chat request, server/RAGHelper_local.py:294-295) with the embeddings and their cosines staying on the device, and the
reference's rerank provenance (server/provenance.py:100-108) beside it, so both methods that need no LLM import from one place.

The reference, restated:
  include_query  true unless the environment variable ``attribute_include_query`` equals ``"False"`` (that name, read at call time).
  s_i            ``cos(doc_i, answer)``, or ``(cos(doc_i, answer) + cos(doc_i, query)) / 2`` with the query included; a zero row gives 0.
  scores         ``s_i / T`` with ``T = s_0 + s_1 + ...`` (left to right) if ``T > 0``, else the ``s_i`` unchanged.
The reference makes three ``SentenceTransformer.encode`` calls and 2 n ``sklearn.cosine_similarity`` calls per request.  Here a request is
ONE forward over (answer, query, contexts) and one kernel over its rows (``rmu_attribution``, include/rmu.h; provenance.hip): fp64 sums in a
fixed order, n doubles cross the bus.  ``compute_similarity_batch`` serves any number of requests that way (the eval scripts attribute
hundreds).

Path choice (as ``MI355XVectorStore._fused_query``):
  native encoder + tokenizer and a shape the host entry point takes   ``rmu_bert_attribute``: token ids in, scores out, one synchronisation
  otherwise, an embedder with ``embed_documents_device``              that tensor, read where it is by ``rmu_attribution``
  any other ``Embeddings`` object                                    ``embed_documents`` and the host-pointer call
All texts of a call share one forward: against the reference's three calls a score moves within the encoder's bf16 batch-shape noise
(include/rmu.h, "Rounding and batch shape").
"""
from __future__ import annotations

import os
from typing import Any, List, Mapping, Optional, Sequence, Tuple

import numpy as np

from . import _native as N

ENV_INCLUDE_QUERY = "attribute_include_query"          # (the reference reads this name, not the template's provenance_include_query)


# ---- pure host functions ------------------------------------------------------------------------------------------------------------------
def include_query_from_env(env: Optional[Mapping[str, str]] = None) -> bool:
    """server/provenance.py:172-174: true unless the variable is the string "False"."""
    env = os.environ if env is None else env
    return env.get(ENV_INCLUDE_QUERY) != "False"


def _text(doc: Any) -> str:
    return doc if isinstance(doc, str) else doc.page_content


def build_request_table(requests: Sequence[Tuple[str, Sequence[Any], str]], include_query: bool):
    """requests = (query, context, answer) each -> (texts, groups [g, 4] int32, the request of each group).  A request with contexts
    contributes the rows answer, query (only with include_query), context 0 .. n - 1 and one group (answer_row, query_row or -1,
    first_doc_row, n); a request without contexts contributes nothing."""
    texts: List[str] = []
    groups, owner = [], []
    for r, (query, context, answer) in enumerate(requests):
        context = list(context)
        if not context:
            continue
        a = len(texts)
        texts.append(answer)
        q = -1
        if include_query:
            q = len(texts)
            texts.append(query)
        first = len(texts)
        texts.extend(_text(d) for d in context)
        groups.append((a, q, first, len(context)))
        owner.append(r)
    return texts, np.asarray(groups, dtype=np.int32).reshape(-1, 4), owner


def _groups_array(groups) -> np.ndarray:
    g = np.ascontiguousarray(np.asarray(groups, dtype=np.int32))
    if g.size == 0:
        return g.reshape(0, 4)
    if g.ndim != 2 or g.shape[1] != 4:
        raise ValueError("attribution: groups is an [n_groups, 4] int32 table (answer_row, query_row or -1, first_doc_row, n_docs)")
    return g


# ---- the device call ----------------------------------------------------------------------------------------------------------------------
def attribution(x, groups, stream: Optional[int] = None):
    """``rmu_attribution``: x [n, dim] fp32 -- a torch CUDA tensor (rows ``x.stride(0)`` floats apart, read where it is, on ``stream`` or
    torch's current stream of its device) or anything numpy can view as a float32 matrix (uploaded) -- and the group table
    -> (scores [sum n_docs], sims [sum n_docs, 2]) numpy float64, packed in group order."""
    lib = N.lib()
    g = _groups_array(groups)
    total = int(np.maximum(g[:, 3], 0).sum()) if len(g) else 0
    scores = np.empty(total, np.float64)
    sims = np.empty((total, 2), np.float64)
    if hasattr(x, "is_cuda") and x.is_cuda:
        import torch
        if x.dim() != 2 or x.dtype != torch.float32:
            raise ValueError("attribution: a 2-d float32 tensor is expected")
        if x.shape[0] > 1 and (x.stride(1) != 1 or x.stride(0) < x.shape[1]):      # (an expanded or overlapping view, like the numpy path)
            x = x.contiguous()
        n, dim = x.shape
        if n == 0 and len(g) == 0:
            return scores, sims
        if stream is None:
            stream = torch.cuda.current_stream(x.device).cuda_stream
        if not stream:
            # torch's null stream: the library would take its own per-thread stream, which is not ordered behind it
            torch.cuda.current_stream(x.device).synchronize()
        with torch.cuda.device(x.device):
            N.check(lib.rmu_attribution(x.data_ptr(), n, dim, x.stride(0) if n > 1 else dim, g.ctypes.data, len(g), N.F_Q_DEVICE,
                                        scores.ctypes.data, sims.ctypes.data, int(stream)), "rmu_attribution")
        return scores, sims
    x = np.asarray(x, dtype=np.float32)
    if x.ndim != 2:
        raise ValueError("attribution: a 2-d float32 array is expected")
    if x.shape[0] > 1 and (x.strides[1] != 4 or x.strides[0] % 4 or x.strides[0] < 4 * x.shape[1]):
        x = np.ascontiguousarray(x)
    n, dim = x.shape
    if n == 0 and len(g) == 0:
        return scores, sims
    N.check(lib.rmu_attribution(x.ctypes.data, n, dim, x.strides[0] // 4 if n > 1 else dim, g.ctypes.data, len(g), 0, scores.ctypes.data,
                                sims.ctypes.data, int(stream or 0)), "rmu_attribution")
    return scores, sims


# ---- the class ----------------------------------------------------------------------------------------------------------------------------
class DocumentSimilarityAttribution:
    """Drop-in for the reference's class on its call site (``self.attributor.compute_similarity(user_query, context, answer)``), over an
    ``Embeddings`` object instead of a SentenceTransformer of its own: ``include_query=None`` reads ``attribute_include_query`` at every
    call, as the reference does; True / False fix it."""

    def __init__(self, embeddings: Any, include_query: Optional[bool] = None):
        self.embeddings = embeddings
        self.include_query = include_query
        self.last_path: Optional[str] = None          # "fused" | "device" | "host": the path the last call took

    def _include_query(self) -> bool:
        return include_query_from_env() if self.include_query is None else bool(self.include_query)

    def _fused(self, texts: List[str], groups: np.ndarray):
        """``rmu_bert_attribute`` when the Embeddings object is the native one and the bucketed shape fits the host entry point; else None."""
        emb = self.embeddings
        can = getattr(emb, "can_tokenize_for_index", None)
        if can is None or not can():
            return None
        ids, lens = emb._tokenize(texts)
        lens = np.minimum(np.asarray(lens, dtype=np.int32), min(ids.shape[1], emb.max_seq_length))
        lmax = max(1, int(lens.max(initial=1)))
        if emb.encoder.host_shape(ids.shape[0], lmax, emb._mode) is None:
            return None
        return emb.encoder.attribute_host(ids[:, :lmax], lens, emb._mode, groups)[0]

    def _scores(self, texts: List[str], groups: np.ndarray) -> np.ndarray:
        got = self._fused(texts, groups)
        if got is not None:
            self.last_path = "fused"
            return got
        dev = getattr(self.embeddings, "embed_documents_device", None)
        if dev is not None:
            self.last_path = "device"
            return attribution(dev(texts), groups)[0]
        e = np.asarray(self.embeddings.embed_documents(texts), dtype=np.float32)
        if e.ndim != 2 or e.shape[0] != len(texts):
            raise ValueError("embed_documents must return one vector per text")
        self.last_path = "host"
        return attribution(e, groups)[0]

    def compute_similarity_batch(self, requests: Sequence[Tuple[str, Sequence[Any], str]]) -> List[List[float]]:
        """(query, context, answer) per request -> the scores of each request's contexts; all requests share one forward and one kernel."""
        requests = list(requests)
        texts, groups, owner = build_request_table(requests, self._include_query())
        out: List[List[float]] = [[] for _ in requests]
        if not owner:
            return out
        scores = self._scores(texts, groups)
        at = 0
        for r, g in zip(owner, groups):
            out[r] = scores[at:at + int(g[3])].tolist()
            at += int(g[3])
        return out

    def compute_similarity(self, query: str, context: Sequence[Any], answer: str) -> List[float]:
        return self.compute_similarity_batch([(query, context, answer)])[0]


MI355XSimilarityAttribution = DocumentSimilarityAttribution


def compute_rerank_provenance(reranker, query, documents, answer):
    """server/provenance.py:100-108: the documents scored against the answer -- against query + "\\n" + answer when ``attribute_include_query``
    is the string "True" (this function's own reading of the variable) -- by the compressor that reranked them."""
    if os.getenv(ENV_INCLUDE_QUERY) == "True":
        full_text = query + "\n" + answer
    else:
        full_text = answer
    return reranker.compress_documents(documents, full_text)
