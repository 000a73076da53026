"""GPU: rerank by key -- the device assembly and selection against their host restatement (tests/rerank_ref.py), the one call against the
two-step path it replaces, bit for bit, and the retriever against the compressor.  Everything is equality: no tolerance anywhere."""
import ctypes
import threading

import numpy as np
import pytest

from tests import helpers, rerank_ref as R

pytestmark = pytest.mark.gpu

CLS, SEP, PAD = 101, 102, 0


def _err(lib):
    return lib.rmu_last_error().decode()


@pytest.fixture(scope="module")
def lib():
    from ragmeup_amd import _native
    lib = _native.lib()
    assert lib.rmu_init(0) == 0, _err(lib)
    return lib


class Table:
    """A native table and the host copy of what was put into it (the tokens before any cut)."""

    def __init__(self, lib, max_len=512):
        self.lib, self.max_len, self.entries = lib, max_len, []
        self.h = ctypes.c_void_p()
        assert lib.rmu_passages_create(ctypes.byref(self.h), CLS, SEP, PAD, max_len) == 0, _err(lib)

    def set(self, first, entries):
        tokens = np.ascontiguousarray(np.concatenate([np.asarray(e, dtype=np.int32) for e in entries] + [np.zeros(0, np.int32)]))
        offsets = np.zeros(len(entries) + 1, dtype=np.int64)
        offsets[1:] = np.cumsum([len(e) for e in entries])
        assert self.lib.rmu_passages_set(self.h, first, tokens.ctypes.data, offsets.ctypes.data, len(entries)) == 0, _err(self.lib)
        self.entries = self.entries[:first] + [np.asarray(e, dtype=np.int32) for e in entries]

    def close(self):
        self.lib.rmu_passages_free(self.h)


def _queries(rng, lens, budget):
    """-> q_tokens [nq, stride] (the heads the pairs can use), q_lens (before any cut), the full token lists"""
    full = [rng.integers(1000, 30000, n).astype(np.int32) for n in lens]
    stride = max(1, max(min(n, budget) for n in lens))
    q = np.zeros((len(lens), stride), dtype=np.int32)
    for i, f in enumerate(full):
        q[i, :min(len(f), stride)] = f[:stride]
    return q, np.asarray(lens, dtype=np.int32), full


def _ref_rows(table, full_q, keys, max_len):
    m = keys.shape[1]
    ids = np.empty((keys.size, max_len), dtype=np.int32)
    types = np.empty_like(ids)
    lens = np.empty(keys.size, dtype=np.int32)
    for r, k in enumerate(keys.reshape(-1)):
        ids[r], types[r], lens[r] = R.assemble(full_q[r // m], None if k < 0 else table.entries[k], max_len, CLS, SEP, PAD)
    return ids, types, lens


def _check_pairs(lib, table, rng, max_len, nq, m, q_lens, key_pool):
    q, ql, full = _queries(rng, q_lens, max_len - 3)
    keys = np.resize(np.asarray(key_pool, dtype=np.int64), (nq, m)).copy()
    ids = np.full((nq * m, max_len), -7, dtype=np.int32)
    types = np.full_like(ids, -7)
    lens = np.full(nq * m, -7, dtype=np.int32)
    rc = lib.rmu_passages_pairs(table.h, q.ctypes.data, ql.ctypes.data, nq, q.shape[1], keys.ctypes.data, m, max_len, ids.ctypes.data,
                                types.ctypes.data, lens.ctypes.data)
    assert rc == 0, _err(lib)
    rid, rty, rlen = _ref_rows(table, full, keys, max_len)
    assert np.array_equal(lens, rlen), (max_len, nq, m)
    assert np.array_equal(ids, rid) and np.array_equal(types, rty), (max_len, nq, m)


def test_pairs_equal_the_restated_assembly(lib):
    """Every (query length, passage length) around the edges of longest_first at max_len 8 / 16 / 512; lists with absent keys, a key twice, key 0
    and the last key; again after a set that makes the device image grow, and after a truncating one."""
    rng = np.random.default_rng(5)
    t = Table(lib)
    lens = sorted({n for ml in (8, 16, 512) for n in R.grid(ml)})
    t.set(0, [rng.integers(1000, 30000, n) for n in lens])
    key_of = {n: i for i, n in enumerate(lens)}

    def sweep():
        last = len(t.entries) - 1
        for max_len in (8, 16, 512):
            g = R.grid(max_len)
            pool = [key_of[n] for n in g if key_of[n] <= last] + [-1, 0, last, last, -1]
            for i in range(0, len(g), 3):                              # every query length against every passage length
                _check_pairs(lib, t, rng, max_len, 3, 14, (g + g)[i:i + 3], pool)
            _check_pairs(lib, t, rng, max_len, 1, 1, [g[3]], [last])
            _check_pairs(lib, t, rng, max_len, 1, 1, [g[-1]], [-1])
            _check_pairs(lib, t, rng, max_len, 1, 65, [g[4]], pool)
            _check_pairs(lib, t, rng, max_len, 3, 256, [g[-1], g[0], g[5]], pool[::-1])
        _check_pairs(lib, t, rng, 64, 1, 256, [20], [-1])               # a list of absent keys only

    sweep()
    grown = len(t.entries)
    t.set(grown, [rng.integers(1000, 30000, int(n)) for n in rng.integers(0, 200, 3000)])     # ~300k tokens: both allocations are outgrown
    sweep()
    _check_pairs(lib, t, rng, 512, 3, 65, [7, 300, 509], list(range(grown - 2, grown + 200, 3)))
    t.set(5, [rng.integers(1000, 30000, n) for n in (13, 600, 0, 2)])   # truncates to 5 entries, then appends four others
    sweep()
    _check_pairs(lib, t, rng, 16, 1, 14, [6], list(range(9)))
    keys = np.array([[9]], dtype=np.int64)                              # one past the end: refused on the host
    q, ql, _ = _queries(rng, [3], 13)
    out = np.zeros(16, dtype=np.int32)
    assert lib.rmu_passages_pairs(t.h, q.ctypes.data, ql.ctypes.data, 1, q.shape[1], keys.ctypes.data, 1, 16, out.ctypes.data, out.ctypes.data,
                                  out.ctypes.data) == -1 and "outside the table" in _err(lib)
    t.close()


def _crafted_logits(rng, nq, m):
    """Per query another hazard: all equal, runs of ties, signed zeros, infinities, NaNs, and plain random values."""
    v = rng.standard_normal((nq, m)).astype(np.float32)
    v[0] = 1.5
    if nq > 1:
        v[1] = np.repeat(rng.standard_normal(m // 4 + 1), 4)[:m]
    if nq > 2:
        v[2] = np.where(np.arange(m) % 2 == 0, 0.0, -0.0)
        v[2, m // 3] = 1e-30
    if nq > 3:
        v[3, ::3] = np.inf
        v[3, 1::5] = -np.inf
    if nq > 4:
        v[4, ::2] = np.nan
        v[4, 1::4] = -np.inf
    if nq > 5:
        v[5] = np.nan
    return v


@pytest.mark.parametrize("m", [1, 63, 64, 65, 255, 256])
def test_select_equals_pythons_stable_sort(lib, m):
    import torch
    rng = np.random.default_rng(m)
    nq = 9
    logits = _crafted_logits(rng, nq, m)
    keys = rng.integers(0, 1000, (nq, m)).astype(np.int64)
    keys[6] = -1                                                        # wholly absent
    keys[7, ::2] = -1                                                   # partly absent
    logits[7, : m // 2] = 0.25                                          # ... with ties across the gaps
    keys[8, rng.integers(0, m, m // 3 + 1)] = -1
    dev = torch.device("cuda", 0)
    side = torch.cuda.Stream(dev)
    for top_n in sorted({1, 3, m, m + 5}):
        want = [R.select(logits[q], keys[q], top_n) for q in range(nq)]
        wpos = np.stack([w[0] for w in want])
        wsc = np.stack([w[1] for w in want])
        pos = np.full((nq, top_n), -9, dtype=np.int32)
        sc = np.full((nq, top_n), 7.0, dtype=np.float32)
        assert lib.rmu_rerank_select(logits.ctypes.data, keys.ctypes.data, nq, m, top_n, 0, pos.ctypes.data, sc.ctypes.data, 0) == 0, _err(lib)
        assert np.array_equal(pos, wpos), (m, top_n)
        assert np.array_equal(sc.view(np.uint32), wsc.view(np.uint32)), (m, top_n)          # the logits' own bits: -0.0, NaN payloads
        # device pointers on a caller's stream: in flight on return
        dl, dk = torch.from_numpy(logits).to(dev), torch.from_numpy(keys).to(dev)
        dpos = torch.full((nq, top_n), -9, dtype=torch.int32, device=dev)
        dsc = torch.full((nq, top_n), 7.0, dtype=torch.float32, device=dev)
        torch.cuda.synchronize(dev)
        assert lib.rmu_rerank_select(dl.data_ptr(), dk.data_ptr(), nq, m, top_n, 3, dpos.data_ptr(), dsc.data_ptr(), side.cuda_stream) == 0, _err(lib)
        side.synchronize()
        assert np.array_equal(dpos.cpu().numpy(), wpos)
        assert np.array_equal(dsc.cpu().numpy().view(np.uint32), wsc.view(np.uint32))
        # mixed: device in, host out
        pos[:] = -9
        assert lib.rmu_rerank_select(dl.data_ptr(), dk.data_ptr(), nq, m, top_n, 1, pos.ctypes.data, sc.ctypes.data, side.cuda_stream) == 0, _err(lib)
        assert np.array_equal(pos, wpos) and np.array_equal(sc.view(np.uint32), wsc.view(np.uint32))


# ---- the one call against the two-step path ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cross():
    from ragmeup_amd.bert import BertEncoder
    w = helpers.bert_weights_numpy(helpers.make_bert(seed=1, layers=2, head=True))
    return BertEncoder(w, layers=2)


def _two_step(enc, table, full_q, keys, bb, lb, top_n, host):
    """The existing path: the restated pairs padded to (bb, lb), rmu_bert_encode_host (host) or rmu_bert_encode, then the restated selection."""
    import torch
    from ragmeup_amd import bert as B
    nq, m = keys.shape
    rid, rty, rlen = _ref_rows(table, full_q, keys, lb)
    ids = np.zeros((bb, lb), dtype=np.int32)
    types = np.zeros((bb, lb), dtype=np.int32)
    lens = np.zeros(bb, dtype=np.int32)
    ids[:nq * m], types[:nq * m], lens[:nq * m] = rid, rty, rlen
    if host:
        logits = np.empty(bb, dtype=np.float32)
        B.N.check(enc._lib.rmu_bert_encode_host(enc._h, ids.ctypes.data, types.ctypes.data, lens.ctypes.data, bb, lb, B.MODE_CE, logits.ctypes.data, 1),
                  "rmu_bert_encode_host")
    else:
        logits = enc.encode_ids(ids, lens, types, mode=B.MODE_CE).cpu().numpy()
    logits = logits[:nq * m].reshape(nq, m)
    sel = [R.select(logits[q], keys[q], top_n) for q in range(nq)]
    return logits, np.stack([s[0] for s in sel]), np.stack([s[1] for s in sel])


def _one_call(enc, table, q, ql, keys, bb, lb, top_n):
    nq, m = keys.shape
    pos = np.full((nq, top_n), -9, dtype=np.int32)
    sc = np.full((nq, top_n), 7.0, dtype=np.float32)
    lg = np.full((nq, m), 7.0, dtype=np.float32)
    rc = enc._lib.rmu_bert_rerank(enc._h, table.h, q.ctypes.data, ql.ctypes.data, nq, q.shape[1], keys.ctypes.data, m, bb, lb, top_n,
                                  pos.ctypes.data, sc.ctypes.data, lg.ctypes.data)
    assert rc == 0, _err(enc._lib)
    return lg, pos, sc


def _same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


@pytest.mark.parametrize("nq,m,bb,lb,host", [(1, 14, 16, 96, True), (1, 1, 1, 64, True), (2, 40, 80, 64, False)],
                         ids=["m14-graph", "m1", "past-4096-tokens"])
def test_one_call_has_the_bits_of_the_two_step_path(lib, cross, nq, m, bb, lb, host):
    """out_logits == rmu_bert_encode_host (rmu_bert_encode past 4096 tokens) over the restated pairs at the same (batch_pad, max_len), bit for
    bit; positions and scores == the restated selection of those logits.  Three calls per shape: eager, capture, replay -- all identical."""
    rng = np.random.default_rng(nq * 1000 + m)
    t = Table(lib)
    t.set(0, [rng.integers(1000, 30000, int(n)) for n in rng.integers(0, 41, 50)])
    q, ql, full = _queries(rng, [int(n) for n in rng.integers(3, 18, nq)], lb - 3)
    keys = rng.integers(0, 50, (nq, m)).astype(np.int64)
    if m > 2:
        keys[0, 1] = -1
        keys[0, 2] = keys[0, 0]                                         # the same passage twice: equal logits, order by position
    top_n = min(m, 5)
    want_lg, want_pos, want_sc = _two_step(cross, t, full, keys, bb, lb, top_n, host)
    present = keys >= 0
    for call in range(3):
        lg, pos, sc = _one_call(cross, t, q, ql, keys, bb, lb, top_n)
        assert _same_bits(lg[present], want_lg[present]), (call, lg, want_lg)
        assert np.array_equal(pos, want_pos) and _same_bits(sc, want_sc), call
    # a table that changed between two calls of one shape: the graph reads the staging buffer, not the table
    t.set(len(t.entries), [rng.integers(1000, 30000, 30)])
    keys[-1, -1] = len(t.entries) - 1
    want_lg, want_pos, want_sc = _two_step(cross, t, full, keys, bb, lb, top_n, host)
    lg, pos, sc = _one_call(cross, t, q, ql, keys, bb, lb, top_n)
    present = keys >= 0
    assert _same_bits(lg[present], want_lg[present]) and np.array_equal(pos, want_pos) and _same_bits(sc, want_sc)
    t.close()


def test_one_call_refuses_what_it_cannot_serve(lib, cross):
    from ragmeup_amd.bert import BertEncoder
    rng = np.random.default_rng(1)
    t = Table(lib, max_len=64)
    t.set(0, [rng.integers(1000, 30000, 5)])
    q, ql, _ = _queries(rng, [4], 61)
    pos = np.zeros(1, dtype=np.int32)
    sc = np.zeros(1, dtype=np.float32)

    def call(enc, key=0, max_len=64):
        keys = np.array([[key]], dtype=np.int64)
        return enc._lib.rmu_bert_rerank(enc._h, t.h, q.ctypes.data, ql.ctypes.data, 1, q.shape[1], keys.ctypes.data, 1, 1, max_len, 1,
                                        pos.ctypes.data, sc.ctypes.data, None)

    assert call(cross) == 0, _err(lib)
    assert call(cross, key=1) == -1 and "outside the table" in _err(lib)
    assert call(cross, max_len=96) == -1 and "max_len" in _err(lib)
    headless = BertEncoder(helpers.bert_weights_numpy(helpers.make_bert(seed=0, layers=1)), layers=1)
    assert call(headless) == -1 and "head" in _err(lib)
    t.close()


# ---- the retriever against the compressor ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ce(tmp_path_factory):
    from ragmeup_amd.embeddings import MI355XCrossEncoder
    d = str(tmp_path_factory.mktemp("ce"))
    helpers.write_ce_checkpoint(d, layers=2)
    return MI355XCrossEncoder(model_dir=d)


class _Base:
    def __init__(self, docs):
        self.docs = docs

    def invoke(self, query):
        return list(self.docs)


def _docs(texts):
    from ragmeup_amd import Document
    return [Document(page_content=t, metadata={"i": i}) for i, t in enumerate(texts)]


def _same_docs(got, want):
    assert [d.page_content for d in got] == [d.page_content for d in want]
    assert [d.metadata for d in got] == [d.metadata for d in want]      # relevance_score: the same floats


def test_the_retriever_returns_what_the_compressor_returns(ce):
    from ragmeup_amd import MI355XRerankRetriever, ScoredCrossEncoderReranker
    from ragmeup_amd import provenance
    texts = helpers.synth_texts(12, seed=11)
    texts += [texts[3], texts[0], " ".join(helpers.synth_texts(30, seed=12, wmin=40))]      # duplicates; one text of far more than 512 tokens
    assert int(ce.tokenizer.encode([texts[-1]], None, max_len=1024)[2][0]) > 512
    docs = _docs(texts)
    comp = ScoredCrossEncoderReranker(model=ce, top_n=5)
    r = MI355XRerankRetriever(base_compressor=comp, base_retriever=_Base(docs))
    query = "which kernel scores the query against the dense index?"
    want = comp.compress_documents(docs, query)
    assert len(want) == 5 and all(isinstance(d.metadata["relevance_score"], float) for d in want)
    before = ce.passages.size()[0]
    _same_docs(r.invoke(query), want)                                    # first sight: the passages are tokenised into the table
    assert ce.passages.size()[0] == before + 13                                   # 15 documents, 13 distinct texts
    _same_docs(r.invoke(query), want)                                    # hit
    _same_docs(r.compress_documents(docs, query), want)
    _same_docs(r.batch_invoke([query, "rerank"])[0], want)
    _same_docs(r.batch_invoke([query, "rerank"])[1], comp.compress_documents(docs, "rerank"))
    # the provenance pass: the same compressor surface, the answer as the query
    answer = "The dense index is scanned by a kernel; " + " ".join(helpers.synth_texts(2, seed=13))
    _same_docs(provenance.compute_rerank_provenance(r, query, docs, answer), provenance.compute_rerank_provenance(comp, query, docs, answer))
    # short texts only: another forward shape (no pair reaches max_seq_length)
    short = _docs(helpers.synth_texts(3, seed=14, wmax=5))
    _same_docs(r.compress_documents(short, "a"), comp.compress_documents(short, "a"))
    # a query longer than the pair budget is the compressor's
    long_q = " ".join(helpers.synth_texts(30, seed=15, wmin=40))
    assert ce.rerank(long_q, texts, 5) is None
    _same_docs(r.compress_documents(docs, long_q), comp.compress_documents(docs, long_q))


def test_two_threads_rerank_on_one_model_and_one_table(ce):
    texts = helpers.synth_texts(14, seed=21, wmax=30)
    queries = [" ".join(t.split()[:6]) for t in helpers.synth_texts(10, seed=22)]
    want = [ce.rerank(q, texts, 4) for q in queries]
    assert all(w is not None and len(w[0]) == 4 for w in want)
    got = [[None] * len(queries) for _ in range(2)]
    errors = []

    def run(slot):
        try:
            for i, q in enumerate(queries):
                got[slot][i] = ce.rerank(q, texts, 4)
        except Exception as e:          # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=run, args=(s,)) for s in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    assert got[0] == want and got[1] == want
