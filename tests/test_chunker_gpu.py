"""GPU: rmu_adjacent_cosine against the fp64 restatement (tests/semantic_ref.py) and against itself, bit for bit; MI355XSemanticChunker over a
stub embedder and over the native encoder.

Kernel tolerance |d - ref| <= 8 * dim * 2**-53: an fp64 sum of `dim` exact products carries a relative error of at most dim * 2**-53 against
the sum of |terms|, which Cauchy-Schwarz bounds by |a| |b|; three such sums (dot, |a|^2, |b|^2) on each side; the factor 8 includes a margin of
2 over those six.  The distances are O(1), so the bound is absolute."""
import numpy as np
import pytest

from tests import semantic_ref as R

pytestmark = pytest.mark.gpu

DIMS = (1, 3, 4, 383, 384, 385, 1024, 3072)
TYPES = ("percentile", "standard_deviation", "interquartile", "gradient")


def _tol(dim):
    return 8 * dim * 2.0 ** -53


def _geometry():
    from ragmeup_amd import _native as N
    return N.ADJ_COS_WAVE_PAIRS, N.ADJ_COS_WG_PAIRS


def _sizes():
    rw, wg = _geometry()
    pairs = sorted({rw - 1, rw, rw + 1, 4 * rw + 1, wg - 1, wg, wg + 1})
    return [1, 2, 3] + [p + 1 for p in pairs if p + 1 > 3]


def _matrix(n, dim, seed):
    return np.random.default_rng(seed).standard_normal((n, dim)).astype(np.float32)


def _cos(x, **kw):
    from ragmeup_amd.chunker import adjacent_cosine
    return adjacent_cosine(x, **kw)


def _bits(a):
    return np.asarray(a, np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def cases():
    """dim -> (matrix of the largest size, its reference distances): every smaller size is a prefix."""
    n = max(_sizes())
    out = {}
    for dim in DIMS:
        x = _matrix(n, dim, 1000 + dim)
        out[dim] = (x, R.distances(x))
    return out


# ---- the kernel against the restatement ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", DIMS)
def test_kernel_equals_the_restatement_host_and_device_pointers(cases, dim):
    import torch
    x, ref = cases[dim]
    xd = torch.from_numpy(x).cuda()
    worst = 0.0
    for n in _sizes():
        for got in (_cos(x[:n]), _cos(xd[:n])):
            assert got.shape == (n - 1,) and got.dtype == np.float64
            if n > 1:
                worst = max(worst, float(np.abs(got - ref[:n - 1]).max()))
        assert np.array_equal(_bits(_cos(x[:n])), _bits(_cos(xd[:n])))
    print(f"dim {dim}: max |d - ref| = {worst:.3e}, bound {_tol(dim):.3e}")
    assert worst <= _tol(dim)


@pytest.mark.parametrize("dim", DIMS)
def test_padded_rows_with_nan_pads_and_a_base_off_by_one_float(cases, dim):
    """stride > dim with NaN in the pad columns (never read), from host and from device pointers; a base one float past a 16-byte boundary:
    the DEVICE tensor takes the 4-byte load path at every width (a host array is uploaded into the aligned workspace, so its offset only
    checks the upload).  All give the bits of the plain call."""
    import torch
    x, ref = cases[dim]
    n = x.shape[0]
    plain = _cos(x)
    assert np.abs(plain - ref).max() <= _tol(dim)
    for pad in (1, 4, 7):
        wide = np.full((n, dim + pad), np.nan, np.float32)
        wide[:, :dim] = x
        assert np.array_equal(_bits(_cos(wide[:, :dim])), _bits(plain)), pad
        wd = torch.from_numpy(wide).cuda()
        assert wd[:, :dim].stride(0) == dim + pad
        assert np.array_equal(_bits(_cos(wd[:, :dim])), _bits(plain)), pad
    flat = np.full(n * dim + 5, np.nan, np.float32)
    flat[1:1 + n * dim] = x.reshape(-1)
    assert np.array_equal(_bits(_cos(flat[1:1 + n * dim].reshape(n, dim))), _bits(plain))
    fd = torch.from_numpy(flat).cuda()
    off = fd[1:1 + n * dim].view(n, dim)
    assert off.data_ptr() % 16 == 4
    assert np.array_equal(_bits(_cos(off)), _bits(plain))
    # a view whose rows overlap (row stride < dim) is copied, on both paths
    if dim > 1 and n * dim >= n + dim:
        assert np.array_equal(_bits(_cos(torch.from_numpy(x.reshape(-1)).cuda().as_strided((n, dim), (1, 1)))),
                              _bits(_cos(np.lib.stride_tricks.as_strided(x.reshape(-1), (n, dim), (4, 4)))))


@pytest.mark.parametrize("dim", DIMS)
def test_zero_rows_nan_rows_and_identical_rows(cases, dim):
    import torch
    rw, _ = _geometry()
    x = cases[dim][0][:2 * rw + 6].copy()
    x[3] = 0.0                       # a zero row
    x[7, dim // 2] = np.nan          # a row holding NaN
    x[11] = x[10]                    # two identical rows
    x[rw + 1] = x[rw]                # ... across a run boundary (pair rw is the first of the second wave)
    x[2 * rw + 3, 0] = np.inf
    ref = R.distances(x)
    for got in (_cos(x), _cos(torch.from_numpy(x).cuda())):
        for i in (2, 3, 6, 7, 2 * rw + 2, 2 * rw + 3):
            assert got[i] == 1.0 and ref[i] == 1.0, i
        for i in (10, rw):
            assert abs(got[i]) <= _tol(dim), (i, got[i])
        assert np.abs(got - ref).max() <= _tol(dim)


def test_a_few_thousand_rows_many_workgroups():
    import torch
    x = _matrix(3001, 384, 77)
    ref = R.distances(x)
    got = _cos(torch.from_numpy(x).cuda())
    print(f"3001 x 384: max |d - ref| = {np.abs(got - ref).max():.3e}")
    assert np.abs(got - ref).max() <= _tol(384)
    assert np.array_equal(_bits(got), _bits(_cos(x)))


def test_caller_stream_with_device_input_and_output(cases):
    import torch
    from ragmeup_amd import _native as N
    lib = N.lib()
    x, ref = cases[384]
    n = x.shape[0]
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        xd = torch.from_numpy(x).cuda()
        out = torch.full((n + 1,), -7.0, dtype=torch.float64, device="cuda")
        s.synchronize()
        N.check(lib.rmu_adjacent_cosine(xd.data_ptr(), n, 384, 384, N.F_Q_DEVICE | N.F_OUT_DEVICE, out.data_ptr(), s.cuda_stream), "rmu_adjacent_cosine")
    s.synchronize()
    got = out.cpu().numpy()
    assert np.array_equal(_bits(got[:n - 1]), _bits(_cos(x)))
    assert (got[n - 1:] == -7.0).all()                      # [n - 1] doubles are written, not one more
    assert np.abs(got[:n - 1] - ref).max() <= _tol(384)
    # the same thread's next call, on the library's own stream, and a host-output call on the caller's stream
    assert np.array_equal(_bits(_cos(xd)), _bits(got[:n - 1]))
    assert np.array_equal(_bits(_cos(xd, stream=s.cuda_stream)), _bits(got[:n - 1]))
    # n == 1: nothing is written
    N.check(lib.rmu_adjacent_cosine(xd.data_ptr(), 1, 384, 384, N.F_Q_DEVICE | N.F_OUT_DEVICE, out.data_ptr(), s.cuda_stream), "rmu_adjacent_cosine")
    s.synchronize()
    assert np.array_equal(_bits(out.cpu().numpy()), _bits(got))


# ---- the kernel against itself, bit for bit -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", (3, 383, 384, 1024, 3072))
def test_a_slice_alone_has_the_bits_it_has_inside_the_full_call(cases, dim):
    import torch
    rw, wg = _geometry()
    x = cases[dim][0]
    n = x.shape[0]
    xd = torch.from_numpy(x).cuda()
    full = _cos(xd)
    for a, b in ((1, n), (rw - 1, rw + 2), (rw + 3, n - 1), (5, 7), (wg - 2, n)):
        assert a % rw != 0 and b - a >= 2
        assert np.array_equal(_bits(_cos(xd[a:b])), _bits(full[a:b - 1])), (a, b)
        assert np.array_equal(_bits(_cos(x[a:b])), _bits(full[a:b - 1])), (a, b)


# ---- the chunker over a stub embedder -------------------------------------------------------------------------------------------------------------
class StubEmbeddings:
    """`embed_documents` only: the chunker takes the host-pointer call."""

    def __init__(self, dim):
        self.dim = dim
        self.calls = 0
        self._cache = {}

    def array(self, texts):
        miss = [t for t in dict.fromkeys(texts) if t not in self._cache]
        if miss:
            for t, v in zip(miss, R.stub_embed(miss, self.dim)):
                self._cache[t] = v
        return np.stack([self._cache[t] for t in texts]) if len(texts) else np.zeros((0, self.dim), np.float32)

    def embed_documents(self, texts):
        self.calls += 1
        return self.array(texts).tolist()

    def embed_query(self, text):
        return self.embed_documents([text])[0]


class StubDeviceEmbeddings(StubEmbeddings):
    """... and with `embed_documents_device`: the chunker reads the tensor where it is."""

    def embed_documents_device(self, texts):
        import torch
        self.calls += 1
        return torch.from_numpy(self.array(texts)).cuda()


LENGTHS = (2, 3, 4, 7, 64, 257)
SEEDS = range(12)


@pytest.fixture(scope="module")
def corpus():
    """The batch: every length x 12 seeds, lengths mixed, a 1-sentence document between the others."""
    texts = []
    for seed in SEEDS:
        for n in LENGTHS:
            texts.append(R.make_document(n, seed))
            texts.append(R.make_document(1, seed * 100 + n))
    return texts


@pytest.fixture(scope="module", params=[(d, c) for d in (384, 1024) for c in (StubEmbeddings, StubDeviceEmbeddings)],
                ids=lambda p: f"{p[0]}-{p[1].__name__}")
def stub(request, corpus):
    """(embedder, per document: sentences, the restatement's own distances)"""
    dim, cls = request.param
    emb = cls(dim)
    ref = []
    for t in corpus:
        s = R.sentences_of(t)
        ref.append((s, R.distances(emb.array(R.windows_of(s, 1))) if len(s) > 1 else np.empty(0)))
    return emb, ref


def _params(kind="percentile", number_of_chunks=None):
    return {"type": kind, "amount": None, "number_of_chunks": number_of_chunks}


ALL_PARAMS = [_params(t) for t in TYPES] + [_params(number_of_chunks=k) for k in (1, 3, 1000)]


def _chunker(emb, p, **kw):
    from ragmeup_amd.chunker import MI355XSemanticChunker
    return MI355XSemanticChunker(emb, breakpoint_threshold_type=p["type"], breakpoint_threshold_amount=p["amount"],
                                 number_of_chunks=p["number_of_chunks"], **kw)


def _split_all(ch, texts):
    """chunks per document from ONE batched call (a distinct metadata per document tells them apart)"""
    from ragmeup_amd import Document
    docs = ch.split_documents([Document(page_content=t, metadata={"i": i}) for i, t in enumerate(texts)])
    out = [[] for _ in texts]
    for d in docs:
        out[d.metadata["i"]].append(d.page_content)
    return out


@pytest.mark.parametrize("p", ALL_PARAMS, ids=lambda p: f"{p['type']}-{p['number_of_chunks']}")
def test_stub_chunks_follow_from_the_returned_distances(stub, corpus, p):
    """(a) exact for every type and number_of_chunks, 3 included: the same doubles go through the same numpy calls."""
    emb, ref = stub
    ch = _chunker(emb, p)
    calls = emb.calls
    got = _split_all(ch, corpus)
    assert emb.calls == calls + 1                                  # ONE embedding call for the whole batch
    dists = ch.distances(corpus)
    for t, chunks, d, (s, d_ref) in zip(corpus, got, dists, ref):
        assert d.dtype == np.float64 and d.shape == ((len(s) - 1,) if R.embedded(s, p) else (0,))
        if d.size:
            assert np.abs(d - d_ref).max() <= _tol(emb.dim)
        assert chunks == R.chunks_from_distances(s, d, p)


@pytest.mark.parametrize("p", [_params(t) for t in TYPES] + [_params(number_of_chunks=k) for k in (1, 1000)],
                         ids=lambda p: f"{p['type']}-{p['number_of_chunks']}")
def test_stub_chunks_equal_the_full_restatement(stub, corpus, p):
    """(b) exact wherever the restatement's own threshold margin is >= 1e-9 -- asserted for every case, never skipped (with this generator
    the smallest margin is 2.6e-5; the kernel's distances differ from numpy's by < 1e-12).  number_of_chunks = 3 is in (a) only: its percentile
    rank is an integer in exact arithmetic, so the threshold sits within an ulp of an element and the last bit of a distance decides."""
    emb, ref = stub
    got = _split_all(_chunker(emb, p), corpus)
    smallest = np.inf
    for chunks, (s, d_ref) in zip(got, ref):
        if R.embedded(s, p):
            m = R.margin_of(d_ref, p)
            smallest = min(smallest, m)
            assert m >= 1e-9
        assert chunks == R.chunks_from_distances(s, d_ref, p)
    print(f"smallest margin {smallest:.3e}")
    # the restatement end to end (split, windows, embed, distances, threshold, assembly) on a sample of every length
    for i in range(0, 4 * len(LENGTHS), 2):
        assert got[i] == R.split_text(corpus[i], emb.array, p)


def test_batched_split_documents_equals_split_text_and_copies_metadata(stub, corpus):
    """(c)"""
    from ragmeup_amd import Document
    emb, _ = stub
    ch = _chunker(emb, _params("percentile"))
    texts = corpus[:24] + ["A b. C d?\n\nE f!  "]
    metas = [{"source": f"doc{i}", "tags": [i]} for i in range(len(texts))]
    docs = ch.split_documents([Document(page_content=t, metadata=m) for t, m in zip(texts, metas)])
    assert docs == ch.create_documents(texts, metadatas=metas) == list(ch.transform_documents([Document(page_content=t, metadata=m)
                                                                                                for t, m in zip(texts, metas)]))
    k = 0
    for t, m in zip(texts, metas):
        for chunk in ch.split_text(t):
            assert docs[k].page_content == chunk and docs[k].metadata == m
            assert docs[k].metadata is not m and docs[k].metadata["tags"] is not m["tags"]      # a deep copy per chunk
            k += 1
    assert k == len(docs)
    for b in (0, 2):
        chb = _chunker(emb, _params("interquartile"), buffer_size=b)
        for t in texts[:12]:
            assert chb.split_text(t) == R.split_text(t, emb.array, _params("interquartile"), buffer_size=b)


# ---- the chunker over the native encoder ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def native(tmp_path_factory):
    from ragmeup_amd.embeddings import MI355XEmbeddings
    from tests.helpers import write_st_checkpoint
    d = str(tmp_path_factory.mktemp("chunker") / "st")
    write_st_checkpoint(d, pooling="mean", normalize=True, max_seq_length=256, layers=6, seed=4, scale=3.0)
    return MI355XEmbeddings(model_dir=d)


def test_native_encoder_two_documents_in_one_call(native):
    texts = [R.make_document(257, 21), R.make_document(7, 22)]
    sents = [R.sentences_of(t) for t in texts]
    windows = [w for s in sents for w in R.windows_of(s, 1)]
    E = native.embed_documents_device(windows).cpu().numpy()
    assert E.shape == (264, 384)
    ref_all = R.distances(E)
    ref = [ref_all[:256], ref_all[257:263]]                        # (pair 256 straddles the two documents)
    for p in ALL_PARAMS:
        ch = _chunker(native, p)
        dists = ch.distances(texts)
        got = _split_all(ch, texts)
        for s, d, r, chunks in zip(sents, dists, ref, got):
            assert d.shape == r.shape
            assert np.abs(d - r).max() <= _tol(384)
            assert chunks == R.chunks_from_distances(s, d, p)
            assert " ".join(chunks) == " ".join(s)
    assert len(_split_all(_chunker(native, _params(number_of_chunks=1000)), texts)[0]) == 256     # a break behind all but the smallest distance
