"""CPU: the semantic chunker's host half (sentence split, windows, thresholds, chunk assembly) against the independent restatement in
tests/semantic_ref.py -- both sides run the same numpy calls on the same doubles, so equality is exact -- the argument validation of
rmu_adjacent_cosine (before any HIP call), and the splitter factory's parsing of the reference's environment variables."""
import ctypes
import itertools

import numpy as np
import pytest

from tests import semantic_ref as R

TYPES = ("percentile", "standard_deviation", "interquartile", "gradient")
PARAMS = [{"type": t, "amount": None, "number_of_chunks": None} for t in TYPES] + \
         [{"type": t, "amount": a, "number_of_chunks": None} for t, a in (("percentile", 50), ("standard_deviation", 1), ("interquartile", 0.5),
                                                                          ("gradient", 60))] + \
         [{"type": "percentile", "amount": None, "number_of_chunks": n} for n in (1, 3, 1000)] + \
         [{"type": "gradient", "amount": None, "number_of_chunks": 3}]


def _ids(p):
    return f"{p['type']}-{p['amount']}-{p['number_of_chunks']}"


def _text(n_sentences, seed=0):
    return R.make_document(n_sentences, seed)


def _product_chunks(sentences, d, p):
    from ragmeup_amd import chunker as C
    return C.chunks_from_distances(sentences, d, p["type"], p["amount"], p["number_of_chunks"])


# ---- ABI ------------------------------------------------------------------------------------------------------------------------------------
def test_adjacent_cosine_rejects_every_invalid_argument_without_a_gpu(librmu):
    x = np.zeros((4, 8), np.float32)
    out = np.zeros(3, np.float64)
    xp, op = x.ctypes.data, out.ctypes.data
    f = librmu.rmu_adjacent_cosine
    bad = {
        "null x": (None, 4, 8, 8, 0, op, 0),
        "null out": (xp, 4, 8, 8, 0, None, 0),
        "unknown flag": (xp, 4, 8, 8, 4, op, 0),
        "unknown high flag": (xp, 4, 8, 8, 1 << 31, op, 0),
        "rows-device flag": (xp, 4, 8, 8, 8, op, 0),
        "dim 0": (xp, 4, 0, 8, 0, op, 0),
        "dim < 0": (xp, 4, -1, 8, 0, op, 0),
        "dim > 3072": (xp, 4, 3073, 4096, 0, op, 0),
        "stride < dim": (xp, 4, 8, 7, 0, op, 0),
        "stride < 0": (xp, 4, 8, -8, 0, op, 0),
        "n 0": (xp, 0, 8, 8, 0, op, 0),
        "n < 0": (xp, -3, 8, 8, 0, op, 0),
        "n * stride overflows": (xp, 1 << 40, 8, 1 << 40, 0, op, 0),
    }
    for what, args in bad.items():
        assert f(*args) == -1, what
        msg = librmu.rmu_last_error()
        assert msg.startswith(b"rmu_adjacent_cosine:") and len(msg) > 24, (what, msg)
    assert (out == 0).all()


def test_adjacent_cosine_one_row_is_no_work(librmu):
    """n == 1: valid, nothing written, nothing launched -- it returns OK on a machine without a GPU."""
    x = np.ones((1, 8), np.float32)
    out = np.full(1, 7.0)
    assert librmu.rmu_adjacent_cosine(x.ctypes.data, 1, 8, 8, 0, out.ctypes.data, 0) == 0
    assert out[0] == 7.0


def test_geometry_constants_match_the_kernel_source():
    import os
    import re
    from ragmeup_amd import _native as N
    src = open(os.path.join(os.path.dirname(N.__file__), "csrc", "semantic.hip")).read()
    assert int(re.search(r"constexpr int kWavePairs = (\d+);", src).group(1)) == N.ADJ_COS_WAVE_PAIRS
    assert int(re.search(r"constexpr int kBlock = (\d+);", src).group(1)) // 64 * N.ADJ_COS_WAVE_PAIRS == N.ADJ_COS_WG_PAIRS


def test_exported_from_the_package():
    import ragmeup_amd
    from ragmeup_amd.chunker import MI355XSemanticChunker
    assert ragmeup_amd.MI355XSemanticChunker is MI355XSemanticChunker and "MI355XSemanticChunker" in ragmeup_amd.__all__
    from ragmeup_amd import _lc
    assert issubclass(MI355XSemanticChunker, _lc.BaseDocumentTransformer)


# ---- sentences and windows --------------------------------------------------------------------------------------------------------------------
def test_sentence_split_keeps_an_empty_last_sentence():
    from ragmeup_amd import chunker as C
    s = C.split_sentences("A b. C d?\n\nE f!  ")
    assert s == ["A b.", "C d?", "E f!", ""] == R.sentences_of("A b. C d?\n\nE f!  ")
    assert C.split_sentences("one sentence without an end") == ["one sentence without an end"]
    assert C.split_sentences("") == [""]
    assert C.split_sentences("a-b-c", "-") == ["a", "b", "c"]


@pytest.mark.parametrize("buffer_size", [0, 1, 2])
@pytest.mark.parametrize("n", [1, 2, 3, 7])
def test_windows_equal_the_restatement(n, buffer_size):
    from ragmeup_amd import chunker as C
    s = R.sentences_of(_text(n))
    assert len(s) == n
    w = C.build_windows(s, buffer_size)
    assert w == R.windows_of(s, buffer_size)
    assert len(w) == n
    if buffer_size == 0:
        assert w == s
    if n == 3 and buffer_size == 1:
        assert w == [s[0] + " " + s[1], s[0] + " " + s[1] + " " + s[2], s[1] + " " + s[2]]
    w = C.build_windows(["A b.", "C d?", "E f!", ""], buffer_size)
    assert w == R.windows_of(["A b.", "C d?", "E f!", ""], buffer_size)
    if buffer_size == 1:
        assert w[-1] == "E f! " and w[-2] == "C d? E f! "


# ---- thresholds and assembly --------------------------------------------------------------------------------------------------------------------
def _distance_arrays(n_pairs):
    rng = np.random.default_rng(100 + n_pairs)
    yield rng.random(n_pairs) * 0.6
    yield np.full(n_pairs, 0.25)                                   # all equal: nothing exceeds any threshold built from them
    d = rng.random(n_pairs) * 0.1
    d[rng.integers(0, n_pairs, max(1, n_pairs // 8))] += 0.7       # a few topic changes
    yield d
    yield np.ones(n_pairs)                                         # what zero / NaN rows give


@pytest.mark.parametrize("p", PARAMS, ids=_ids)
@pytest.mark.parametrize("n", [1, 2, 3, 4, 7, 64, 257])
def test_thresholds_and_chunks_equal_the_restatement(n, p):
    from ragmeup_amd import chunker as C
    s = R.sentences_of(_text(n, seed=3))
    for d in _distance_arrays(max(n - 1, 1)):
        if n == 1:
            d = d[:0]
        want = R.chunks_from_distances(s, d, p)
        got = _product_chunks(s, d.copy(), p)
        assert got == want
        assert " ".join(got) == " ".join(s)                       # chunks partition the sentences in order
        if R.embedded(s, p):
            thr, arr = C.breakpoint_threshold(d, p["type"], p["amount"], p["number_of_chunks"])
            rthr, rarr = R.threshold_of(d, p)
            assert np.float64(thr).tobytes() == np.float64(rthr).tobytes()
            assert np.asarray(arr, np.float64).tobytes() == np.asarray(rarr, np.float64).tobytes()
        else:
            assert got == s


def test_short_texts_are_not_embedded():
    from ragmeup_amd import chunker as C

    class Never:
        def embed_documents(self, texts):
            raise AssertionError("embedded")

        embed_query = embed_documents

    one, two = _text(1), _text(2)
    for t in TYPES:
        ch = C.MI355XSemanticChunker(Never(), breakpoint_threshold_type=t)
        assert ch.split_text(one) == [one]
        assert [d.size for d in ch.distances([one, one])] == [0, 0]
    ch = C.MI355XSemanticChunker(Never(), breakpoint_threshold_type="gradient")
    assert ch.split_text(two) == R.sentences_of(two) and len(ch.split_text(two)) == 2
    ch = C.MI355XSemanticChunker(Never(), breakpoint_threshold_type="gradient", number_of_chunks=1)
    assert ch.split_text(two) == R.sentences_of(two)
    docs = ch.create_documents([one, two], metadatas=[{"source": "a"}, {"source": "b"}])
    assert [d.page_content for d in docs] == [one] + R.sentences_of(two)
    assert [d.metadata for d in docs] == [{"source": "a"}, {"source": "b"}, {"source": "b"}]


def test_number_of_chunks_extremes_and_all_equal_distances():
    from ragmeup_amd import chunker as C
    s = R.sentences_of(_text(7, seed=5))
    d = np.array([0.1, 0.5, 0.2, 0.9, 0.3, 0.4])
    assert C.chunks_from_distances(s, d, number_of_chunks=1) == [" ".join(s)]                      # threshold = the maximum
    got = C.chunks_from_distances(s, d, number_of_chunks=1000)                                    # threshold = the minimum: a break behind all but d[0]
    assert got == [s[0] + " " + s[1], s[2], s[3], s[4], s[5], s[6]]
    for t in TYPES:
        assert C.chunks_from_distances(s, np.full(6, 0.3), t) == [" ".join(s)]


def test_constructor_surface():
    from ragmeup_amd import chunker as C
    ch = C.MI355XSemanticChunker(object())
    assert (ch.buffer_size, ch.breakpoint_threshold_type, ch.breakpoint_threshold_amount, ch.number_of_chunks) == (1, "percentile", 95, None)
    assert ch.sentence_split_regex == r"(?<=[.?!])\s+"
    for t, a in (("percentile", 95), ("standard_deviation", 3), ("interquartile", 1.5), ("gradient", 95)):
        assert C.MI355XSemanticChunker(object(), breakpoint_threshold_type=t).breakpoint_threshold_amount == a
    assert C.MI355XSemanticChunker(object(), breakpoint_threshold_amount=80).breakpoint_threshold_amount == 80
    with pytest.raises(NotImplementedError):
        C.MI355XSemanticChunker(object(), add_start_index=True)
    with pytest.raises(ValueError):
        C.MI355XSemanticChunker(object(), breakpoint_threshold_type="median")
    for m in ("split_text", "create_documents", "split_documents", "transform_documents", "distances"):
        assert callable(getattr(ch, m))


# ---- factory ------------------------------------------------------------------------------------------------------------------------------------
def _reference_parse(env):
    """server/RAGHelper.py:73-76, over a mapping instead of os.environ."""
    amount = int(env.get("breakpoint_threshold_amount")) if env.get("breakpoint_threshold_amount", "None") != "None" else None
    value = env.get("number_of_chunks", None)
    chunks = None if value is None or value.lower() == "none" else int(value)
    return env.get("breakpoint_threshold_type"), amount, chunks


@pytest.mark.parametrize("amount,chunks", list(itertools.product([None, "None", "95", "3"], [None, "None", "none", "NONE", "4"])))
def test_factory_parses_the_environment_like_the_reference(amount, chunks):
    from ragmeup_amd import factory
    from ragmeup_amd.chunker import BREAKPOINT_DEFAULTS, MI355XSemanticChunker
    env = {"splitter": "SemanticChunker", "breakpoint_threshold_type": "interquartile"}
    if amount is not None:
        env["breakpoint_threshold_amount"] = amount
    if chunks is not None:
        env["number_of_chunks"] = chunks
    emb = object()
    ch = factory.text_splitter_from_env(emb, env)
    kind, want_amount, want_chunks = _reference_parse(env)
    assert isinstance(ch, MI355XSemanticChunker) and ch.embeddings is emb
    assert ch.breakpoint_threshold_type == kind == "interquartile"
    assert ch.breakpoint_threshold_amount == (BREAKPOINT_DEFAULTS[kind] if want_amount is None else want_amount)
    assert ch.number_of_chunks == want_chunks and (want_chunks is None or isinstance(want_chunks, int))


def test_factory_rejects_what_the_reference_rejects_and_the_recursive_splitter():
    from ragmeup_amd import factory
    with pytest.raises(ValueError):                                # int('1.5'), as RAGHelper.py:73
        factory.text_splitter_from_env(object(), {"splitter": "SemanticChunker", "breakpoint_threshold_type": "interquartile",
                                                  "breakpoint_threshold_amount": "1.5"})
    with pytest.raises(ValueError):                                # 'none' is None for number_of_chunks only
        factory.text_splitter_from_env(object(), {"splitter": "SemanticChunker", "breakpoint_threshold_type": "percentile",
                                                  "breakpoint_threshold_amount": "none"})
    for kind in ("RecursiveCharacterTextSplitter", None, "semanticchunker"):
        env = {} if kind is None else {"splitter": kind}
        with pytest.raises(ValueError, match="RecursiveCharacterTextSplitter"):
            factory.text_splitter_from_env(object(), env)
