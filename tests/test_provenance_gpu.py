"""GPU: rmu_attribution against the fp64 restatement (tests/provenance_ref.py) and against itself, bit for bit; rmu_bert_attribute against
rmu_bert_encode_host + rmu_attribution; DocumentSimilarityAttribution over a stub embedder (the golden's arrays) and over the native encoder.

Kernel tolerance (the project's rule, tests/test_chunker_gpu.py): |sim - ref| <= tol = 8 * dim * 2**-53 -- an fp64 sum of `dim` exact products
carries a relative error of at most dim * 2**-53 against the sum of |terms|, which Cauchy-Schwarz bounds by |a| |b|; three such sums on each
side, a margin of 2.  An unnormalised score (T <= 0) is a similarity or the mean of two: tol.  A normalised score s / T, |s| <= 1, T the sum of n
scores each within tol: tol / |T| for its own error + n tol / T**2 for the sum's: tol * (1 / |T| + n / T**2), T from the restatement.  Inputs
are seeded so that the restatement alone has |T| >= 0.25 in every group that is normalised, which the tests assert."""
import os

import numpy as np
import pytest

from tests import provenance_ref as R

pytestmark = pytest.mark.gpu

DIMS = (1, 3, 4, 255, 256, 257, 512, 513, 1024, 1025, 2048, 2049, 3071, 3072)        # both sides of every instantiation edge (NJ 1, 2, 4, 8, 12)
SIZES = (0, 1, 2, 63, 64, 65)
N_ROWS = 2 + 65 + 3


def _tol(dim):
    return 8 * dim * 2.0 ** -53


def _bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.uint64)


def _attr(x, groups, **kw):
    from ragmeup_amd.provenance import attribution
    return attribution(x, groups, **kw)


def _matrix(dim, seed):
    """Rows with positive elements at very different scales: every cosine is positive, so no group's T comes near 0 (at dim 1 every
    cosine is 1).  Odd dims are negated as a whole, which changes no cosine."""
    rng = np.random.default_rng(seed)
    x = np.abs(rng.standard_normal((N_ROWS, dim))) * np.exp(rng.uniform(-3, 3, (N_ROWS, 1)))
    return (x if dim % 2 == 0 else -x).astype(np.float32)


def _groups():
    """Rows 0 / 1: answer / query.  Every size with and without a query, the documents at different first rows (so rows are shared between
    groups); group sizes 65 start at row 0 / 1: their first document is their own anchor; the last two groups take anchors from the middle."""
    g = []
    for i, n in enumerate(SIZES):
        first = 2 + (i % 3) if n < 65 else 0
        g.append((0, 1, first, n))
        g.append((0, -1, first + 1 if n < 65 else 1, n))
    g.append((40, 41, 39, 5))                              # anchors inside their own documents
    g.append((N_ROWS - 1, -1, N_ROWS - 3, 3))              # the last rows of the matrix
    return np.asarray(g, dtype=np.int32)


def _check(scores, sims, ref, groups, dim, what=""):
    """against the restatement's (scores, sims, totals); -> the worst excess ratios"""
    rs, rm, totals = ref
    assert scores.shape == rs.shape and sims.shape == rm.shape and scores.dtype == sims.dtype == np.float64
    tol = _tol(dim)
    worst_sim = float(np.abs(sims - rm).max(initial=0.0))
    assert worst_sim <= tol, (what, worst_sim, tol)
    at = 0
    worst = 0.0
    for (a, q, first, n), t in zip(groups, totals):
        if n == 0:
            continue
        if t > 0:
            assert abs(t) >= 0.25, (what, t)
            bound = tol * (1 / abs(t) + n / t ** 2)
        else:
            bound = tol
        err = float(np.abs(scores[at:at + n] - rs[at:at + n]).max())
        assert err <= bound, (what, (a, q, first, n), err, bound)
        worst = max(worst, err / bound)
        at += n
    assert at == len(scores)
    return worst_sim / tol, worst


@pytest.fixture(scope="module")
def cases():
    """dim -> (matrix, group table, the restatement's outputs), computed once"""
    out = {}
    g = _groups()
    for dim in DIMS:
        x = _matrix(dim, 2000 + dim)
        out[dim] = (x, g, R.attribute_groups(x, g))
    return out


def _device_view(x, stride, offset, fill=np.nan):
    """x as a device tensor whose rows are `stride` floats apart and whose base is `offset` floats past an aligned address; every float
    that is not an element of x is `fill`"""
    import torch
    n, dim = x.shape
    flat = np.full(offset + n * stride + 8, fill, np.float32)
    for r in range(n):
        flat[offset + r * stride:offset + r * stride + dim] = x[r]
    t = torch.from_numpy(flat).cuda()
    v = t[offset:offset + n * stride].view(n, stride)[:, :dim]
    assert v.data_ptr() % 16 == 4 * (offset % 4) and (v.stride(0) == stride or n == 1)
    return v


# ---- (a) the kernel against the restatement -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", DIMS)
def test_kernel_equals_the_restatement_at_every_width_alignment_and_group_size(cases, dim):
    x, g, ref = cases[dim]
    assert sorted(set(g[:, 3].tolist())) == [0, 1, 2, 3, 5, 63, 64, 65]
    first = None
    for stride in (dim, dim + 1):
        for offset in (0, 1):
            scores, sims = _attr(_device_view(x, stride, offset), g)
            w = _check(scores, sims, ref, g, dim, (stride, offset))
            if first is None:
                first = (scores, sims)
                print(f"dim {dim}: worst |sim - ref| / tol = {w[0]:.3f}, worst |score - ref| / bound = {w[1]:.3f}")
            # (b) the 16-byte path (stride a multiple of 4, aligned base) and the 4-byte path give the same bits
            assert np.array_equal(_bits(scores), _bits(first[0])) and np.array_equal(_bits(sims), _bits(first[1])), (stride, offset)
    # (b) host x (uploaded) against device x; a host array with padded rows
    hs, hm = _attr(x, g)
    assert np.array_equal(_bits(hs), _bits(first[0])) and np.array_equal(_bits(hm), _bits(first[1]))
    wide = np.full((x.shape[0], dim + 3), np.nan, np.float32)
    wide[:, :dim] = x
    hs, hm = _attr(wide[:, :dim], g)
    assert np.array_equal(_bits(hs), _bits(first[0])) and np.array_equal(_bits(hm), _bits(first[1]))
    # without a query the second similarity is +0.0
    at = 0
    for a, q, f, n in g:
        if q < 0:
            assert (_bits(first[1][at:at + n, 1]) == 0).all()
        at += n


# ---- (b) the kernel against itself, bit for bit ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", (3, 255, 256, 513, 1025, 2049, 3072))
def test_a_group_alone_has_the_bits_it_has_inside_the_larger_call(cases, dim):
    import torch
    x, g, _ = cases[dim]
    full_s, full_m = _attr(torch.from_numpy(x).cuda(), g)
    at = 0
    for a, q, first, n in g.tolist():
        if n in (1, 2, 5, 64, 65):
            # the group's rows alone, in another order: documents first, then the query, then the answer
            rows = list(range(first, first + n)) + ([q] if q >= 0 else []) + [a]
            alone = np.ascontiguousarray(x[rows])
            ga = [[len(rows) - 1, n if q >= 0 else -1, 0, n]]
            for arg in (alone, torch.from_numpy(alone).cuda()):
                s, m = _attr(arg, ga)
                assert np.array_equal(_bits(s), _bits(full_s[at:at + n])), (a, q, first, n)
                assert np.array_equal(_bits(m), _bits(full_m[at:at + n])), (a, q, first, n)
        at += n
    # the same table in reverse order: every group keeps its bits
    rs, rm = _attr(x, g[::-1].copy())
    ends = np.cumsum(g[:, 3])
    back = np.concatenate([np.arange(e - n, e) for e, n in zip(ends[::-1], g[::-1, 3])]) if len(g) else []
    assert np.array_equal(_bits(rs), _bits(full_s[back])) and np.array_equal(_bits(rm), _bits(full_m[back]))


def test_device_outputs_on_a_caller_stream_and_no_similarities(cases):
    """RMU_F_OUT_DEVICE on a torch stream: drained on return (no synchronisation by the caller); exactly sum n_docs doubles are written;
    out_sims may be NULL."""
    import torch
    from ragmeup_amd import _native as N
    lib = N.lib()
    x, g, _ = cases[513]
    want_s, want_m = _attr(x, g)
    total = int(g[:, 3].sum())
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        xd = torch.from_numpy(x).cuda()
        out = torch.full((total + 1,), -7.0, dtype=torch.float64, device="cuda")
        sims = torch.full((total + 1, 2), -7.0, dtype=torch.float64, device="cuda")
        s.synchronize()
        N.check(lib.rmu_attribution(xd.data_ptr(), x.shape[0], 513, 513, g.ctypes.data, len(g), N.F_Q_DEVICE | N.F_OUT_DEVICE, out.data_ptr(),
                                    sims.data_ptr(), s.cuda_stream), "rmu_attribution")
        assert s.query()                                   # the call drained the stream
        got_s, got_m = out.cpu().numpy(), sims.cpu().numpy()
        assert np.array_equal(_bits(got_s[:total]), _bits(want_s)) and np.array_equal(_bits(got_m[:total]), _bits(want_m))
        assert got_s[total] == -7.0 and (got_m[total] == -7.0).all()
        out.fill_(-7.0)
        s.synchronize()
        N.check(lib.rmu_attribution(xd.data_ptr(), x.shape[0], 513, 513, g.ctypes.data, len(g), N.F_Q_DEVICE | N.F_OUT_DEVICE, out.data_ptr(),
                                    None, s.cuda_stream), "rmu_attribution")
        assert np.array_equal(_bits(out.cpu().numpy()[:total]), _bits(want_s))
    host = np.full(total, -7.0)
    N.check(lib.rmu_attribution(x.ctypes.data, x.shape[0], 513, 513, g.ctypes.data, len(g), 0, host.ctypes.data, None, 0), "rmu_attribution")
    assert np.array_equal(_bits(host), _bits(want_s))


# ---- (c) sign and degenerate cases ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", (4, 384, 3072))
def test_negative_and_zero_totals_zero_rows_and_nan(dim):
    import torch
    rng = np.random.default_rng(300 + dim)
    x = np.abs(rng.standard_normal((24, dim))).astype(np.float32)
    x[2:8] *= -1                     # documents opposed to both anchors: T < 0
    x[8:12] = 0.0                    # all contexts zero: T == 0
    x[12] = 0.0                      # a zero answer row (anchor of the fifth group)
    x[14] = 0.0                      # a zero document row among others
    x[17, dim // 2] = np.nan         # a NaN element in a document
    x[22, dim - 1] = np.nan          # a NaN element in an answer (anchor of the last group)
    g = np.asarray([(0, 1, 2, 6), (0, -1, 2, 6), (0, 1, 8, 4), (0, -1, 8, 4), (12, 1, 18, 4), (12, -1, 18, 4), (0, 1, 13, 6), (22, 1, 18, 3)],
                   dtype=np.int32)
    ref = R.attribute_groups(x, g)
    totals = ref[2]
    assert totals[0] < -0.25 and totals[1] < -0.25 and totals[2] == 0.0 and totals[3] == 0.0 and totals[5] == 0.0
    for arg in (x, torch.from_numpy(x).cuda()):
        s, m = _attr(arg, g)
        _check(s, m, ref, g, dim)
        ends = np.cumsum(g[:, 3])
        part = lambda a, i: a[ends[i] - g[i, 3]:ends[i]]
        # T < 0: the unnormalised similarities come back
        assert np.array_equal(_bits(part(s, 0)), _bits((part(m, 0)[:, 0] + part(m, 0)[:, 1]) / 2)) and (part(s, 0) < 0).all()
        assert np.array_equal(_bits(part(s, 1)), _bits(part(m, 1)[:, 0])) and (part(s, 1) < 0).all()
        # T == 0, all contexts zero: zeros (+0.0)
        for i in (2, 3, 5):
            assert (_bits(part(s, i)) == 0).all() and (_bits(part(m, i)) == 0).all(), i
        # a zero answer with a query: the answer's similarity is 0, the score is the query's half, normalised
        assert (part(m, 4)[:, 0] == 0).all() and (part(m, 4)[:, 1] > 0).all()
        assert abs(part(s, 4).sum() - 1.0) <= 1e-12
        # a zero document and a document with a NaN element count as similarity 0 and take no share
        for row in (14, 17):
            assert part(s, 6)[row - 13] == 0.0 and (part(m, 6)[row - 13] == 0).all()
        assert abs(part(s, 6).sum() - 1.0) <= 1e-12 and (np.delete(part(s, 6), (1, 4)) > 0).all()
        # a NaN element in the answer: only the query's similarity is left
        assert (part(m, 7)[:, 0] == 0).all() and (part(m, 7)[:, 1] > 0).all()
        assert not np.isnan(s).any() and not np.isnan(m).any()


# ---- (d) the fused entry point --------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def native(tmp_path_factory):
    from ragmeup_amd.embeddings import MI355XEmbeddings
    from tests.helpers import write_st_checkpoint
    d = str(tmp_path_factory.mktemp("provenance") / "st")
    write_st_checkpoint(d, pooling="mean", normalize=True, max_seq_length=512, layers=6, seed=4, scale=3.0)
    return MI355XEmbeddings(model_dir=d)


def _requests(seed, sizes, wmax=30):
    from tests.helpers import synth_texts
    texts = synth_texts(2 * len(sizes) + sum(sizes), seed=seed, wmin=4, wmax=wmax)
    out, at = [], 0
    for n in sizes:
        out.append((texts[at], texts[at + 2:at + 2 + n], texts[at + 1]))
        at += 2 + n
    return out


@pytest.mark.parametrize("sizes,include_query", [((10,), True), ((3,), False), ((10, 4), True), ((1, 0, 5), False)])
def test_fused_call_equals_encode_then_attribution(native, sizes, include_query):
    """rmu_bert_attribute against rmu_bert_encode_host on the same bucketed shape followed by rmu_attribution on the vectors it returns:
    scores, similarities and out_vecs bit for bit; eager, capture and replay of the shape."""
    enc = native.encoder
    texts, groups = R.request_rows(_requests(5, sizes), include_query)
    groups = np.asarray(groups, dtype=np.int32)
    ids, lens = native._tokenize(texts)
    assert enc.host_shape(ids.shape[0], ids.shape[1], native._mode) is not None
    for rep in range(3):
        v = enc.encode_host(ids, lens, None, mode=native._mode)
        want_s, want_m = _attr(v, groups)
        got_s, got_m, got_v = enc.attribute_host(ids, lens, native._mode, groups, want_vectors=True)
        assert got_v.shape == (len(texts), 384) and np.array_equal(got_v, v), rep
        assert len(got_s) == sum(sizes)
        assert np.array_equal(_bits(got_s), _bits(want_s)) and np.array_equal(_bits(got_m), _bits(want_m)), rep
    # a table that names a row beyond the batch is refused before the forward
    bad = groups.copy()
    bad[0, 3] += len(texts)
    with pytest.raises(Exception):
        enc.attribute_host(ids, lens, native._mode, bad)


# ---- (e) the class --------------------------------------------------------------------------------------------------------------------------------
class GoldenEmbeddings:
    """`embed_documents` only, serving the golden's arrays by text: the class takes the host-pointer call."""

    def __init__(self):
        self.rows = {}
        self.calls = 0

    def embed_documents(self, texts):
        self.calls += 1
        return [self.rows[t].tolist() for t in texts]


class GoldenDeviceEmbeddings(GoldenEmbeddings):
    def embed_documents_device(self, texts):
        import torch
        self.calls += 1
        return torch.from_numpy(np.stack([self.rows[t] for t in texts])).cuda()


def _golden():
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "provenance_golden.npz"))
    return [{"name": str(name), "answer": z[f"c{i}_answer"], "query": z[f"c{i}_query"], "docs": z[f"c{i}_docs"],
             "include_query": bool(z[f"c{i}_include_query"]), "out": z[f"c{i}_out"]} for i, name in enumerate(z["names"])]


@pytest.mark.parametrize("cls,path", [(GoldenEmbeddings, "host"), (GoldenDeviceEmbeddings, "device")])
def test_class_over_the_golden_arrays(monkeypatch, cls, path):
    """Within (a)'s tolerance of the restatement, hence within the CPU test's bound of the reference's outputs (asserted too); one request
    per call with the variable set as the reference reads it, then all requests of one setting in one batch."""
    from ragmeup_amd.provenance import DocumentSimilarityAttribution
    emb = cls()
    a = DocumentSimilarityAttribution(emb)
    requests = {True: [], False: []}
    single = {True: [], False: []}
    for c in _golden():
        name, n = c["name"], len(c["docs"])
        emb.rows[name + " answer"], emb.rows[name + " query"] = c["answer"], c["query"]
        context = [f"{name} context {j}" for j in range(n)]
        for t, row in zip(context, c["docs"]):
            emb.rows[t] = row
        monkeypatch.setenv("attribute_include_query", "True" if c["include_query"] else "False")
        calls = emb.calls
        got = a.compute_similarity(name + " query", context, name + " answer")
        assert emb.calls == calls + 1 and a.last_path == path
        assert isinstance(got, list) and len(got) == n and all(isinstance(v, float) for v in got)
        want, _, total = R.attribute(c["docs"], c["answer"], c["query"] if c["include_query"] else None)
        tol = _tol(384)
        bound = tol * (1 / abs(total) + n / total ** 2) if total > 0 else tol
        assert np.abs(np.asarray(got) - want).max() <= bound, name
        eps32 = (2 * 384 + 8) * 2.0 ** -24
        assert np.abs(np.asarray(got) - c["out"].astype(np.float64)).max() <= (eps32 * (1 / abs(total) + n / total ** 2) if total > 0 else eps32) + bound
        requests[c["include_query"]].append((name + " query", context, name + " answer"))
        single[c["include_query"]].append(got)
    for include_query in (True, False):
        batch = DocumentSimilarityAttribution(emb, include_query=include_query).compute_similarity_batch(requests[include_query] + [("q", [], "a")])
        assert batch[-1] == [] and batch[:-1] == single[include_query]          # a group has the same bits wherever it sits


def test_class_over_the_native_encoder_fused_path_equals_the_two_call_path(native, monkeypatch):
    from ragmeup_amd.provenance import DocumentSimilarityAttribution
    monkeypatch.delenv("attribute_include_query", raising=False)
    a = DocumentSimilarityAttribution(native)
    for sizes in ((10,), (2, 7)):
        requests = _requests(11, sizes)
        got = a.compute_similarity_batch(requests)
        assert a.last_path == "fused" and [len(s) for s in got] == list(sizes)
        texts, groups = R.request_rows(requests, True)
        ids, lens = native._tokenize(texts)
        v = native.encoder.encode_host(ids, lens, None, mode=native._mode)
        want = _attr(v, groups)[0]
        assert np.array_equal(_bits(np.concatenate(got)), _bits(want))
        for s in got:
            assert abs(sum(s) - 1.0) <= 1e-12
    q, context, answer = requests[1]
    assert a.compute_similarity(q, context, answer) == a.compute_similarity(q, [type("D", (), {"page_content": t})() for t in context], answer)
    assert a.compute_similarity(q, [], answer) == []
    monkeypatch.setenv("attribute_include_query", "False")
    off = a.compute_similarity(q, context, answer)
    assert a.last_path == "fused" and len(off) == len(context) and off != got[1]


def test_class_takes_the_device_tensor_path_when_the_request_is_too_large_for_the_host_entry_point(native):
    """12 texts bucketed to 512 tokens: 6144 tokens, more than the host entry point's 4096.  The scores must equal the restatement applied to
    the embeddings embed_documents_device returns, within (a)'s tolerance."""
    from ragmeup_amd.provenance import DocumentSimilarityAttribution
    from tests.helpers import synth_texts
    request = _requests(17, (10,))[0]
    request = (request[0], [synth_texts(1, seed=99, wmin=600, wmax=600)[0]] + list(request[1][1:]), request[2])
    texts, groups = R.request_rows([request], True)
    assert len(texts) == 12
    ids, lens = native._tokenize(texts)
    assert int(lens.max()) > 480 and native.encoder.host_shape(12, int(lens.max()), native._mode) is None
    a = DocumentSimilarityAttribution(native, include_query=True)
    got = np.asarray(a.compute_similarity(*request))
    assert a.last_path == "device" and got.shape == (10,)
    E = native.embed_documents_device(texts).cpu().numpy()
    want, _, total = R.attribute(E[2:], E[0], E[1])
    err = float(np.abs(got - want).max())
    bound = _tol(384) * (1 / abs(total) + 10 / total ** 2) if total > 0 else _tol(384)
    print(f"T = {total:.4f}, max |score - ref| = {err:.3e}, bound {bound:.3e}")
    assert err <= bound
