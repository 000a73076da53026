"""MI355XSemanticChunker -- the reference's second splitter, ``SemanticChunker(self.embeddings, breakpoint_threshold_type=...,
breakpoint_threshold_amount=..., number_of_chunks=...)`` (server/RAGHelper.py:329-349, built when ``splitter=SemanticChunker``), with the
window embeddings and their distances staying on the device.

langchain_experimental 0.0.64 (the reference's pin) is restated here:
  sentences  ``re.split(sentence_split_regex, text)``, default ``(?<=[.?!])\\s+``; an empty last sentence (text that ends in punctuation and
             whitespace) is kept.  One sentence -> ``[that sentence]``; two sentences with type ``gradient`` -> the two sentences; neither
             is embedded.
  windows    sentence i joined with the ``buffer_size`` sentences in front of it (each followed by " ") and behind it (each led by " ").
  distances  ``1 - cosine_similarity`` of the embeddings of windows i and i + 1: ``rmu_adjacent_cosine`` (include/rmu.h; semantic.hip), one
             fp64 per pair, computed where the embeddings are.
  threshold  ``number_of_chunks`` given: the percentile of the distances that the linear map (len(d) chunks -> 0, 1 chunk -> 100) assigns
             to it; else by type -- ``percentile`` (amount 95), ``standard_deviation`` (mean + 3 std), ``interquartile``
             (mean + 1.5 (q3 - q1)), ``gradient`` (percentile 95 of ``np.gradient`` of the distances, which is then the compared array).
  chunks     a break behind every sentence i whose array[i] > threshold; chunk = the sentences between two breaks joined by " ".
The thresholds stay host numpy on the n - 1 doubles the device returns: an order statistic of that few numbers has nothing to gain there.

One call does the whole batch: ``create_documents`` / ``split_documents`` gather the windows of ALL texts into one list, make one
``embed_documents_device`` call (the embedder's pipeline tokenises behind the forward) and one ``rmu_adjacent_cosine`` over the tensor; the
pairs that straddle two documents are dropped on the host.  All windows of a call therefore share one forward: against a per-document call a
breakpoint can move where a distance sits within the encoder's bf16 batch-shape noise of the threshold (include/rmu.h, "Rounding and batch
shape").  An ``Embeddings`` object without ``embed_documents_device`` is served through ``embed_documents`` and a host-pointer call.

Not built: ``add_start_index`` (raises) and ``min_chunk_size``.
"""
from __future__ import annotations

import copy
import re
from typing import Any, Iterable, List, Optional, Sequence

import numpy as np

from . import _native as N
from ._lc import BaseDocumentTransformer, Document

BREAKPOINT_DEFAULTS = {"percentile": 95, "standard_deviation": 3, "interquartile": 1.5, "gradient": 95}
DEFAULT_SENTENCE_SPLIT_REGEX = r"(?<=[.?!])\s+"


# ---- pure host functions ----------------------------------------------------------------------------------------------------------------
def split_sentences(text: str, sentence_split_regex: str = DEFAULT_SENTENCE_SPLIT_REGEX) -> List[str]:
    return re.split(sentence_split_regex, text)


def build_windows(sentences: Sequence[str], buffer_size: int = 1) -> List[str]:
    """The text that is embedded for sentence i: the sentences i - buffer_size .. i + buffer_size that exist, joined by single spaces."""
    n = len(sentences)
    out = []
    for i in range(n):
        w = ""
        for j in range(i - buffer_size, i):
            if j >= 0:
                w += sentences[j] + " "
        w += sentences[i]
        for j in range(i + 1, i + 1 + buffer_size):
            if j < n:
                w += " " + sentences[j]
        out.append(w)
    return out


def needs_embedding(sentences: Sequence[str], breakpoint_threshold_type: str) -> bool:
    if len(sentences) == 1:
        return False
    return not (breakpoint_threshold_type == "gradient" and len(sentences) == 2)


def breakpoint_threshold(distances, breakpoint_threshold_type: str = "percentile", breakpoint_threshold_amount: Optional[float] = None,
                         number_of_chunks: Optional[int] = None):
    """-> (threshold, the array that is compared with it)."""
    d = distances
    if number_of_chunks is not None:
        x1 = len(d)
        x = max(min(number_of_chunks, x1), 1.0)
        y = 100.0 if x1 == 1 else 0.0 + (100.0 / (1.0 - x1)) * (x - x1)
        y = min(max(y, 0), 100)
        return np.percentile(d, y), d
    if breakpoint_threshold_type not in BREAKPOINT_DEFAULTS:
        raise ValueError(f"Got unexpected `breakpoint_threshold_type`: {breakpoint_threshold_type}")
    amount = BREAKPOINT_DEFAULTS[breakpoint_threshold_type] if breakpoint_threshold_amount is None else breakpoint_threshold_amount
    if breakpoint_threshold_type == "percentile":
        return np.percentile(d, amount), d
    if breakpoint_threshold_type == "standard_deviation":
        return np.mean(d) + amount * np.std(d), d
    if breakpoint_threshold_type == "interquartile":
        q1, q3 = np.percentile(d, [25, 75])
        return np.mean(d) + amount * (q3 - q1), d
    g = np.gradient(d, range(len(d)))
    return np.percentile(g, amount), g


def assemble_chunks(sentences: Sequence[str], array, threshold) -> List[str]:
    chunks = []
    start = 0
    for i in [i for i, v in enumerate(array) if v > threshold]:
        chunks.append(" ".join(sentences[start:i + 1]))
        start = i + 1
    if start < len(sentences):
        chunks.append(" ".join(sentences[start:]))
    return chunks


def chunks_from_distances(sentences: Sequence[str], distances, breakpoint_threshold_type: str = "percentile",
                          breakpoint_threshold_amount: Optional[float] = None, number_of_chunks: Optional[int] = None) -> List[str]:
    """The chunks of one text given the distances of its windows (ignored where the text is not embedded)."""
    if not needs_embedding(sentences, breakpoint_threshold_type):
        return list(sentences)
    thr, arr = breakpoint_threshold(distances, breakpoint_threshold_type, breakpoint_threshold_amount, number_of_chunks)
    return assemble_chunks(sentences, arr, thr)


# ---- the device call ----------------------------------------------------------------------------------------------------------------------
def adjacent_cosine(x, stream: Optional[int] = None) -> np.ndarray:
    """``rmu_adjacent_cosine``: x [n, dim] fp32 -- a torch CUDA tensor (rows ``x.stride(0)`` floats apart, read where it is, on ``stream`` or
    torch's current stream of its device) or anything numpy can view as a float32 matrix (uploaded) -> numpy float64 [n - 1]."""
    lib = N.lib()
    if hasattr(x, "is_cuda") and x.is_cuda:
        import torch
        if x.dim() != 2 or x.dtype != torch.float32:
            raise ValueError("adjacent_cosine: a 2-d float32 tensor is expected")
        if x.shape[0] > 1 and (x.stride(1) != 1 or x.stride(0) < x.shape[1]):      # (an expanded or overlapping view, like the numpy path)
            x = x.contiguous()
        n, dim = x.shape
        out = np.empty(max(n - 1, 0), np.float64)
        if n < 2:
            return out
        if stream is None:
            stream = torch.cuda.current_stream(x.device).cuda_stream
        if not stream:
            # torch's null stream: the library would take its own per-thread stream, which is not ordered behind it
            torch.cuda.current_stream(x.device).synchronize()
        with torch.cuda.device(x.device):
            N.check(lib.rmu_adjacent_cosine(x.data_ptr(), n, dim, x.stride(0), N.F_Q_DEVICE, out.ctypes.data, int(stream)), "rmu_adjacent_cosine")
        return out
    x = np.asarray(x, dtype=np.float32)
    if x.ndim != 2:
        raise ValueError("adjacent_cosine: a 2-d float32 array is expected")
    if x.shape[0] > 1 and (x.strides[1] != 4 or x.strides[0] % 4 or x.strides[0] < 4 * x.shape[1]):
        x = np.ascontiguousarray(x)
    n, dim = x.shape
    out = np.empty(max(n - 1, 0), np.float64)
    if n < 2:
        return out
    N.check(lib.rmu_adjacent_cosine(x.ctypes.data, n, dim, x.strides[0] // 4, 0, out.ctypes.data, int(stream or 0)), "rmu_adjacent_cosine")
    return out


# ---- the splitter -------------------------------------------------------------------------------------------------------------------------
class MI355XSemanticChunker(BaseDocumentTransformer):
    """Drop-in for ``langchain_experimental.text_splitter.SemanticChunker`` on the reference's call site: same constructor names and
    defaults, ``split_text`` / ``create_documents`` / ``split_documents`` / ``transform_documents``.  All windows of one call share one
    forward (module docstring): a breakpoint can differ from a per-document call's where a distance lies within the encoder's bf16
    batch-shape noise of the threshold."""

    def __init__(self, embeddings: Any, buffer_size: int = 1, add_start_index: bool = False,
                 breakpoint_threshold_type: str = "percentile", breakpoint_threshold_amount: Optional[float] = None,
                 number_of_chunks: Optional[int] = None, sentence_split_regex: str = DEFAULT_SENTENCE_SPLIT_REGEX):
        if add_start_index:
            raise NotImplementedError("MI355XSemanticChunker: add_start_index is not built")
        if breakpoint_threshold_type not in BREAKPOINT_DEFAULTS:
            raise ValueError(f"Got unexpected `breakpoint_threshold_type`: {breakpoint_threshold_type}")
        self._add_start_index = False
        self.embeddings = embeddings
        self.buffer_size = int(buffer_size)
        self.breakpoint_threshold_type = breakpoint_threshold_type
        self.number_of_chunks = number_of_chunks
        self.sentence_split_regex = sentence_split_regex
        self.breakpoint_threshold_amount = (BREAKPOINT_DEFAULTS[breakpoint_threshold_type] if breakpoint_threshold_amount is None
                                            else breakpoint_threshold_amount)

    # ---- the batch: one forward, one distance call ------------------------------------------------------------------------------------
    def _embed(self, windows: List[str]):
        dev = getattr(self.embeddings, "embed_documents_device", None)
        if dev is not None:
            return dev(windows)
        e = np.asarray(self.embeddings.embed_documents(windows), dtype=np.float32)
        if e.ndim != 2 or e.shape[0] != len(windows):
            raise ValueError("embed_documents must return one vector per text")
        return e

    def _sentences_and_distances(self, texts: Iterable[str]):
        sents = [split_sentences(t, self.sentence_split_regex) for t in texts]
        windows: List[str] = []
        spans = []
        for s in sents:
            if needs_embedding(s, self.breakpoint_threshold_type):
                spans.append((len(windows), len(s)))
                windows.extend(build_windows(s, self.buffer_size))
            else:
                spans.append(None)
        d_all = adjacent_cosine(self._embed(windows)) if windows else np.empty(0, np.float64)
        # the pair (last window of a text, first window of the next) is not a pair of any text: dropped here
        dists = [np.empty(0, np.float64) if sp is None else d_all[sp[0]:sp[0] + sp[1] - 1].copy() for sp in spans]
        return sents, dists

    def distances(self, texts: Sequence[str]) -> List[np.ndarray]:
        """The fp64 distances of every text's adjacent windows (an empty array for a text that is not embedded), from one batch call."""
        return self._sentences_and_distances(list(texts))[1]

    def _split_batch(self, texts: List[str]) -> List[List[str]]:
        sents, dists = self._sentences_and_distances(texts)
        return [chunks_from_distances(s, d, self.breakpoint_threshold_type, self.breakpoint_threshold_amount, self.number_of_chunks)
                for s, d in zip(sents, dists)]

    # ---- LangChain's surface ----------------------------------------------------------------------------------------------------------------
    def split_text(self, text: str) -> List[str]:
        return self._split_batch([text])[0]

    def create_documents(self, texts: List[str], metadatas: Optional[List[dict]] = None) -> List[Document]:
        texts = list(texts)
        metas = metadatas or [{}] * len(texts)
        docs = []
        for i, chunks in enumerate(self._split_batch(texts)):
            for chunk in chunks:
                docs.append(Document(page_content=chunk, metadata=copy.deepcopy(metas[i])))
        return docs

    def split_documents(self, documents: Iterable[Document]) -> List[Document]:
        texts, metas = [], []
        for d in documents:
            texts.append(d.page_content)
            metas.append(d.metadata)
        return self.create_documents(texts, metadatas=metas)

    def transform_documents(self, documents: Sequence[Document], **kwargs: Any) -> Sequence[Document]:
        return self.split_documents(list(documents))
