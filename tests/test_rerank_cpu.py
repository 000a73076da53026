"""CPU: rerank by key without a device -- the restated assembly against the tokenizer, the passage table's host side, every argument error,
the text -> key dictionary, and the retriever's fallbacks."""
import ctypes
import os

import numpy as np
import pytest

from tests import helpers, rerank_ref as R


@pytest.fixture(scope="module")
def tok(librmu, tmp_path_factory):
    from ragmeup_amd.tokenizer import WordPieceTokenizer
    d = tmp_path_factory.mktemp("rerank_vocab")
    helpers._write_tokenizer_files(str(d))
    return WordPieceTokenizer(os.path.join(str(d), "vocab.txt"))


def _text(n, shift=0):
    """n single-letter words: n tokens of the synthetic vocabulary."""
    return " ".join(chr(ord("a") + (i + shift) % 26) for i in range(n))


def _tokens(tok, texts):
    """Each text tokenised on its own, without special tokens and without a cut."""
    L = max(len(t.split()) for t in texts) + 2
    ids, _, lens = tok.encode(texts, None, max_len=max(L, 3))
    return [ids[i, 1:lens[i] - 1].copy() for i in range(len(texts))]


def _err(lib):
    return lib.rmu_last_error().decode()


@pytest.mark.parametrize("max_len", [8, 16, 512])
def test_assembly_restated_equals_the_tokenizer_over_the_length_grid(tok, max_len):
    """rerank_ref.assemble over separately tokenised texts == WordPieceTokenizer.encode(a, b, max_len): id, type and length, at every pair of
    lengths around the edges of longest_first (both parities of the split, equal lengths on both sides of the budget)."""
    cls, sep, pad = (int(v) for v in tok.encode([""], None, max_len=8)[0][0, :3])
    g = R.grid(max_len)
    assert len(g) == 9 or max_len == 8          # (max_len 8: b = 5, some edges coincide)
    pairs = [(la, lb) for la in g for lb in g]
    ta = [_text(la) for la, _ in pairs]
    tb = [_text(lb, shift=7) for _, lb in pairs]
    ids, types, lens = tok.encode(ta, tb, max_len=max_len)
    qa, pb = _tokens(tok, ta), _tokens(tok, tb)
    for i, (la, lb) in enumerate(pairs):
        assert len(qa[i]) == la and len(pb[i]) == lb
        rid, rty, rlen = R.assemble(qa[i], pb[i], max_len, cls, sep, pad)
        assert rlen == lens[i], (la, lb)
        assert np.array_equal(rid, ids[i]) and np.array_equal(rty, types[i]), (la, lb)


def _table(lib, max_len=16, cls=101, sep=102, pad=0):
    h = ctypes.c_void_p()
    assert lib.rmu_passages_create(ctypes.byref(h), cls, sep, pad, max_len) == 0, _err(lib)
    return h


def _set(lib, h, first, entries):
    tokens = np.array([t for e in entries for t in e], dtype=np.int32)
    offsets = np.zeros(len(entries) + 1, dtype=np.int64)
    offsets[1:] = np.cumsum([len(e) for e in entries])
    return lib.rmu_passages_set(h, first, tokens.ctypes.data if tokens.size else None, offsets.ctypes.data, len(entries))


def _size(lib, h):
    n, t = ctypes.c_int64(-1), ctypes.c_int64(-1)
    assert lib.rmu_passages_size(h, ctypes.byref(n), ctypes.byref(t)) == 0
    return n.value, t.value


def test_table_bookkeeping_without_a_device(librmu):
    lib = librmu
    h = ctypes.c_void_p()
    for bad in (7, 513, 0, -1):
        assert lib.rmu_passages_create(ctypes.byref(h), 101, 102, 0, bad) == -1
        assert "max_len" in _err(lib)
    assert lib.rmu_passages_create(None, 101, 102, 0, 16) == -1
    h = _table(lib, max_len=16)                                   # entries keep 13 tokens
    assert _size(lib, h) == (0, 0)
    assert _set(lib, h, 0, [[5, 6, 7], [], [8] * 13, [9] * 14, [10] * 40]) == 0, _err(lib)
    assert _size(lib, h) == (5, 3 + 0 + 13 + 13 + 13)             # an entry longer than max_len - 3 keeps its head
    assert _set(lib, h, 5, [[1, 2]]) == 0                         # append
    assert _size(lib, h) == (6, 44)
    assert _set(lib, h, 2, [[3]]) == 0                            # first < size truncates, then appends
    assert _size(lib, h) == (3, 4)
    assert _set(lib, h, 1, []) == 0                               # n = 0 only truncates
    assert _size(lib, h) == (1, 3)
    # each failure changes nothing
    assert _set(lib, h, 2, [[1]]) == -1 and "out of step" in _err(lib)
    assert _set(lib, h, -1, [[1]]) == -1
    assert _set(lib, h, 1, [[1, -2, 3]]) == -1 and "negative" in _err(lib)
    tokens = np.arange(4, dtype=np.int32)
    desc = np.array([0, 3, 2], dtype=np.int64)
    assert lib.rmu_passages_set(h, 1, tokens.ctypes.data, desc.ctypes.data, 2) == -1 and "ascend" in _err(lib)
    from1 = np.array([1, 3], dtype=np.int64)
    assert lib.rmu_passages_set(h, 1, tokens.ctypes.data, from1.ctypes.data, 1) == -1 and "start at 0" in _err(lib)
    assert lib.rmu_passages_set(None, 0, tokens.ctypes.data, desc.ctypes.data, 0) == -1
    assert lib.rmu_passages_size(None, None, None) == -1
    assert _size(lib, h) == (1, 3)
    assert lib.rmu_passages_free(h) == 0
    assert lib.rmu_passages_free(None) == 0


def test_every_argument_error_returns_before_a_device_is_touched(librmu):
    lib = librmu
    h = _table(lib, max_len=16)
    assert _set(lib, h, 0, [[5, 6, 7], [8, 9]]) == 0
    q = np.array([[11, 12, 13, 14]], dtype=np.int32)
    ql = np.array([4], dtype=np.int32)
    keys = np.array([[0, 1, -1]], dtype=np.int64)
    ids = np.zeros((3, 16), dtype=np.int32)
    ty = np.zeros((3, 16), dtype=np.int32)
    ln = np.zeros(3, dtype=np.int32)
    P = lambda a: a.ctypes.data      # noqa: E731

    def pairs(p=h, qt=P(q), qlen=P(ql), nq=1, stride=4, k=P(keys), m=3, max_len=16, o1=P(ids), o2=P(ty), o3=P(ln)):
        return lib.rmu_passages_pairs(p, qt, qlen, nq, stride, k, m, max_len, o1, o2, o3)

    for kw in ({"p": None}, {"qt": None}, {"qlen": None}, {"k": None}, {"o1": None}, {"o2": None}, {"o3": None}):
        assert pairs(**kw) == -1 and "null" in _err(lib), kw
    for kw in ({"m": 0}, {"m": 257}, {"nq": 0}, {"stride": 0}, {"max_len": 7}, {"max_len": 17}):
        assert pairs(**kw) == -1, kw
    assert pairs(k=P(np.array([[0, 2, -1]], dtype=np.int64))) == -1 and "outside the table" in _err(lib)      # key >= size
    assert pairs(k=P(np.array([[0, -2, 1]], dtype=np.int64))) == -1
    assert pairs(qlen=P(np.array([-1], dtype=np.int32))) == -1
    assert pairs(qlen=P(np.array([9], dtype=np.int32))) == -1 and "q_stride" in _err(lib)     # the row does not hold the query's head

    lg = np.zeros((1, 3), dtype=np.float32)
    pos = np.zeros(2, dtype=np.int32)
    sc = np.zeros(2, dtype=np.float32)

    def select(l=P(lg), k=P(keys), nq=1, m=3, top_n=2, flags=0, o1=P(pos), o2=P(sc)):
        return lib.rmu_rerank_select(l, k, nq, m, top_n, flags, o1, o2, 0)

    for kw in ({"l": None}, {"k": None}, {"o1": None}, {"o2": None}):
        assert select(**kw) == -1 and "null" in _err(lib), kw
    for kw in ({"m": 0}, {"m": 257}, {"top_n": 0}, {"nq": 0}, {"flags": 4}):
        assert select(**kw) == -1, kw

    lo = np.zeros((1, 3), dtype=np.float32)

    def rerank(model=None, p=h, qt=P(q), qlen=P(ql), nq=1, stride=4, k=P(keys), m=3, batch_pad=4, max_len=16, top_n=2, o1=P(pos), o2=P(sc)):
        return lib.rmu_bert_rerank(model, p, qt, qlen, nq, stride, k, m, batch_pad, max_len, top_n, o1, o2, P(lo))

    for kw in ({"m": 0}, {"m": 257}):
        assert rerank(**kw) == -1 and "m_cand" in _err(lib), kw
    assert rerank(top_n=0) == -1 and "top_n" in _err(lib)
    for kw in ({"p": None}, {"qt": None}, {"qlen": None}, {"k": None}, {"o1": None}, {"o2": None}):
        assert rerank(**kw) == -1 and "null" in _err(lib), kw
    assert rerank(batch_pad=2) == -1 and "batch_pad" in _err(lib)
    assert rerank(max_len=17) == -1 and "max_len" in _err(lib)
    assert rerank(k=P(np.array([[0, 2, -1]], dtype=np.int64))) == -1 and "outside the table" in _err(lib)     # key >= size
    assert rerank() == -1 and "null" in _err(lib)                  # everything else in order: the model is missing
    assert lib.rmu_passages_free(h) == 0


def test_passage_table_numbers_distinct_texts_and_refills_at_its_cap(tok):
    from ragmeup_amd.rerank import PassageTable
    t = PassageTable.for_tokenizer(tok, max_len=16, max_entries=4)
    calls = []

    class Counting:
        def encode(self, a, b, max_len):
            calls.append(list(a))
            return tok.encode(a, b, max_len=max_len)

    k = t.keys_for(["a b c", "d e", "a b c", _text(30)], Counting())
    assert k.tolist() == [0, 1, 0, 2] and k.dtype == np.int64
    assert calls == [["a b c", "d e", _text(30)]]                 # one tokenizer call, each new text once
    assert t.size() == (3, 3 + 2 + 13) and len(t) == 3
    assert t.keys_for(["d e", "a b c"], Counting()).tolist() == [1, 0] and len(calls) == 1      # hits tokenise nothing
    t.warm(["f g"], Counting())
    assert t.size() == (4, 20) and t.clears == 0
    # the cap: table and dictionary are cleared, the call's texts refill them
    assert t.keys_for(["d e", "h", "h"], Counting()).tolist() == [0, 1, 1]
    assert t.clears == 1 and t.size() == (2, 3) and calls[-1] == ["d e", "h"]
    assert t.keys_for(["a b c"], Counting()).tolist() == [2]
    t.close()


def _docs(texts):
    from ragmeup_amd import Document
    return [Document(page_content=t, metadata={"i": i}) for i, t in enumerate(texts)]


class _Base:
    def __init__(self, docs):
        self.docs = docs

    def invoke(self, query):
        return list(self.docs)


def _score(pairs):
    return [float((len(q) * 7 + len(p) * 13) % 5) for q, p in pairs]       # ties included


def _stub_cross_encoder(tok, activation):
    """An MI355XCrossEncoder in everything `rerank` looks at before it reaches the device."""
    from ragmeup_amd.bert import BertEncoder
    from ragmeup_amd.embeddings import MI355XCrossEncoder
    ce = object.__new__(MI355XCrossEncoder)
    ce.encoder = object.__new__(BertEncoder)
    ce.tokenizer, ce.activation, ce.max_seq_length, ce.token_budget = tok, activation, 512, 1 << 20
    ce.score = _score
    return ce


class _Plain:
    score = staticmethod(_score)


@pytest.mark.parametrize("case", ["sigmoid", "empty", "too_many", "not_native"])
def test_the_retriever_falls_back_to_the_compressor(tok, case):
    from ragmeup_amd import MI355XRerankRetriever, ScoredCrossEncoderReranker
    texts = helpers.synth_texts(300 if case == "too_many" else 9, seed=3, wmax=6)
    model = _Plain() if case == "not_native" else _stub_cross_encoder(tok, "sigmoid" if case == "sigmoid" else "identity")
    docs = [] if case == "empty" else _docs(texts)
    comp = ScoredCrossEncoderReranker(model=model, top_n=4)
    r = MI355XRerankRetriever(base_compressor=comp, base_retriever=_Base(docs))
    want = comp.compress_documents(docs, "what is a query?")
    assert len(want) == (0 if case == "empty" else 4)
    for got in (r.compress_documents(docs, "what is a query?"), r.invoke("what is a query?"), r.batch_invoke(["what is a query?"])[0]):
        assert [(d.page_content, d.metadata) for d in got] == [(d.page_content, d.metadata) for d in want]
