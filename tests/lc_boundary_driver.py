"""Runs the LangChain side of the drop-in boundary with `ragmeup_amd._lc.HAVE_LANGCHAIN` True: the third-party
modules are replaced by tests/lcstub.py stand-ins that keep LangChain's pydantic `isinstance` field validation, and our objects
are wired the way a LangChain application wires a vector store, a BM25 + dense ensemble and a cross-encoder compressor.
Executed in a fresh interpreter by tests/test_boundary_cpu.py (the package resolves its LangChain base classes at import
time).  Prints one JSON object.
"""
import hashlib
import json
import os
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import lcstub  # noqa: E402

lcstub.install()

import numpy as np  # noqa: E402

import ragmeup_amd  # noqa: E402,F401
from ragmeup_amd import _lc  # noqa: E402
from ragmeup_amd.vectorstore import MI355XRetriever, MI355XVectorStore  # noqa: E402

out = {"have_langchain": _lc.HAVE_LANGCHAIN}
assert _lc.HAVE_LANGCHAIN and _lc.Document is lcstub.Document

# ---- CPU stand-ins for the two GPU models (the boundary, not the arithmetic, is under test here) --------------------------
from test_host_cpu import FakeStore  # noqa: E402  (MI355XVectorStore over an oracle-backed index: a TEST subclass)

from ragmeup_amd.embeddings import MI355XCrossEncoder, MI355XEmbeddings  # noqa: E402
from ragmeup_amd.reranker import ScoredCrossEncoderReranker as OurReranker  # noqa: E402


class HashEmbeddings(MI355XEmbeddings):
    """MI355XEmbeddings with the encoder replaced by a hash (same class hierarchy -> same isinstance answers)."""

    def __init__(self):
        pass

    def embed_documents_array(self, texts):
        rows = []
        for t in texts:
            seed = int(hashlib.md5(t.replace("\n", " ").encode()).hexdigest()[:8], 16)
            v = np.random.default_rng(seed).standard_normal(384)
            rows.append(v / np.linalg.norm(v))
        return np.asarray(rows, dtype=np.float32)

    embed_documents_device = None

    def embed_documents(self, texts):
        return self.embed_documents_array(texts).tolist()


class OverlapCrossEncoder(MI355XCrossEncoder):
    def __init__(self, model_name=None):
        self.model_name = model_name

    def score(self, text_pairs):
        return [float(len(set(a.lower().split()) & set(b.lower().split()))) + 1e-4 * (int(hashlib.md5(b.encode()).hexdigest()[:4], 16) % 97)
                for a, b in text_pairs]


del HashEmbeddings.embed_documents_device
emb = HashEmbeddings()
out["embeddings_is_Embeddings"] = isinstance(emb, lcstub.Embeddings)
out["cross_encoder_is_both_bases"] = (isinstance(OverlapCrossEncoder(), lcstub.BaseCrossEncoder)
                                      and isinstance(OverlapCrossEncoder(), lcstub.CommunityBaseCrossEncoder))
out["semantic_chunker_ok"] = lcstub.SemanticChunker(emb).embeddings is emb          # type-checks Embeddings

# ---- store: an empty collection, then 2300 chunks in 1000-document add_documents calls with md5 ids ----------------------
tmp = tempfile.mkdtemp()
env = {"vector_store_uri": os.path.join(tmp, "data.db"), "vector_store_collection": "ragmeup_documents", "vector_store_k": "4"}
topics = ["alpha", "beta", "gamma", "delta", "epsilon"]
chunks = []
for i in range(2300):
    text = f"chunk {i} about {topics[i % 5]} and {topics[(i // 5) % 5]} number {i * 7919 % 1000}"
    chunks.append(lcstub.Document(page_content=text, metadata={"source": f"{topics[i % 5]}.pdf", "id": hashlib.md5(text.encode()).hexdigest()}))
db = FakeStore.from_documents([], emb, drop_old=True, connection_args={"uri": env["vector_store_uri"]},
                              collection_name=env["vector_store_collection"])
for lo in range(0, len(chunks), 1000):
    batch = chunks[lo:lo + 1000]
    db.add_documents(batch, ids=[d.metadata["id"] for d in batch])
out["db_type"] = [c.__name__ for c in type(db).__mro__ if c.__module__.startswith("ragmeup_amd.")][0]
out["db_rows"] = len(db)
out["db_is_VectorStore"] = isinstance(db, lcstub.VectorStore)


# ---- retrievers: BM25 + the store's mmr retriever in an EnsembleRetriever, our reranker in a ContextualCompressionRetriever
def build_retrievers(store, docs):
    sparse = lcstub.BM25Retriever.from_texts([d.page_content for d in docs], metadatas=[d.metadata for d in docs], k=4)
    dense = store.as_retriever(search_type="mmr", search_kwargs={"k": int(env["vector_store_k"])})
    return sparse, dense, lcstub.EnsembleRetriever(retrievers=[sparse, dense], weights=[0.5, 0.5])


sparse, dense, ensemble = build_retrievers(db, chunks)
out["dense_type"] = type(dense).__name__
out["dense_is_VectorStoreRetriever"] = isinstance(dense, lcstub.VectorStoreRetriever) and isinstance(dense, MI355XRetriever)
compressor = OurReranker(model=OverlapCrossEncoder(), top_n=3)
rerank_retriever = lcstub.ContextualCompressionRetriever(base_compressor=compressor, base_retriever=ensemble)
out["compressor_is_BaseDocumentCompressor"] = isinstance(compressor, lcstub.BaseDocumentCompressor)
out["rerank_retriever_type"] = type(rerank_retriever).__name__

query = "what about gamma and delta number 57"
ens_docs = ensemble.invoke(query)
out["ensemble_n"] = len(ens_docs)
out["ensemble_has_pk"] = all("pk" in d.metadata for d in dense.invoke(query))
rr_docs = rerank_retriever.invoke(query)
out["rerank_n"] = len(rr_docs)
out["rerank_scores_desc"] = [d.metadata["relevance_score"] for d in rr_docs]
out["rerank_keeps_source_id"] = all("source" in d.metadata and "id" in d.metadata for d in rr_docs)

# expected result, recomputed independently: same members, scored by the same model, stable sort, top_n
exp = sorted(((d, s) for d, s in zip(ens_docs, OverlapCrossEncoder().score([(query, d.page_content) for d in ens_docs]))),
             key=lambda p: p[1], reverse=True)[:3]
out["rerank_matches_expected"] = [d.page_content for d in rr_docs] == [d.page_content for d, _ in exp]


def format_documents(docs):
    return "\n\n".join(f"Document {i} content: {d.page_content}" for i, d in enumerate(docs))


# LCEL compositions: `retriever | function` and a dict coerced to a parallel step
out["pipe_format_ok"] = (rerank_retriever | format_documents).invoke(query).startswith("Document 0 content: ")
par = {"docs": ensemble, "context": ensemble | format_documents, "question": lcstub.RunnablePassthrough()} | lcstub.RunnableLambda(lambda d: d)
res = par.invoke(query)
out["dict_coercion_ok"] = sorted(res) == ["context", "docs", "question"] and len(res["docs"]) == len(ens_docs)


# strictness of the stand-ins and of our reranker: a duck-typed object must be rejected (otherwise the test above proves nothing)
class Duck:
    def invoke(self, q, config=None):
        return []

    def score(self, pairs):
        return [0.0] * len(pairs)

    def compress_documents(self, documents, query, callbacks=None):
        return documents


rejected = []
for label, make in (("ensemble", lambda: lcstub.EnsembleRetriever(retrievers=[sparse, Duck()], weights=[0.5, 0.5])),
                    ("compression", lambda: lcstub.ContextualCompressionRetriever(base_compressor=Duck(), base_retriever=ensemble)),
                    ("our_reranker", lambda: OurReranker(model=Duck(), top_n=3)),
                    ("our_reranker_extra", lambda: OurReranker(model=OverlapCrossEncoder(), bogus=1))):
    try:
        make()
    except Exception:  # noqa: BLE001
        rejected.append(label)
out["duck_rejected"] = rejected

# incremental add (retrievers rebuilt over the grown store) and delete by source
new = [lcstub.Document(page_content="a brand new chunk about zeta", metadata={"source": "zeta.pdf", "id": "z1"})]
db.add_documents(new, ids=[d.metadata["id"] for d in new])
chunks += new
_, _, ensemble2 = build_retrievers(db, chunks)
out["after_add_rows"] = len(db)
out["new_dense_type"] = type(ensemble2.retrievers[1]).__name__
out["finds_new"] = any(d.metadata.get("source") == "zeta.pdf" for d in db.similarity_search("a brand new chunk about zeta", k=1))
out["delete_count"] = db.delete(expr='source == "alpha.pdf"').delete_count

# env factory (ragmeup_amd.factory): vector_store=mi355x
from ragmeup_amd import factory  # noqa: E402

fenv = dict(env, vector_store="mi355x", vector_store_initial_load="True", rerank="False",
            vector_store_collection="factory_probe")   # a fresh collection: the product class itself (index built lazily)


class _Rec:                      # the logger an application hands to its helper: anything with .info / .error
    def __init__(self):
        self.lines = []

    def info(self, m):
        self.lines.append(("info", str(m)))

    def error(self, m):
        self.lines.append(("error", str(m)))

    warning = info


rec = _Rec()
hp = factory.from_env(fenv, embeddings=HashEmbeddings(), logger=rec)
out["factory_logged"] = [m for _, m in rec.lines]
from ragmeup_amd import _log  # noqa: E402

out["logger_injected"] = _log.get_logger() is rec
_log.set_logger(None)
out["factory_db"] = type(hp.db).__name__
out["factory_is_MI355XVectorStore"] = isinstance(hp.db, MI355XVectorStore)
out["factory_retriever"] = [hp.retriever.search_type, hp.retriever.search_kwargs]
out["factory_compressor"] = hp.compressor
try:
    factory.embeddings_from_env(dict(fenv, force_cpu="True", embedding_model=tmp))
    out["force_cpu_raises"] = False
except RuntimeError:
    out["force_cpu_raises"] = True

print("RESULT " + json.dumps(out))
