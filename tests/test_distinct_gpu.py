"""GPU: the grouped search (rmu_index_search_distinct: scan_distinct_kernel + k_distinct_fold) against the host reference of
tests/distinct_ref.py -- every live row ranked with the chain scores of tests/exact_regimes.py, walked greedily by code.  Every comparison
is exact: row ids equal, scores equal as uint32 (E.mismatch).  The corpora are built here so that the code layouts can be placed by the
planner's own numbers (R.plan): floods that cross tile, row-part and workgroup-chunk boundaries, bit-identical rows, ties at rank k."""
from dataclasses import dataclass
from functools import lru_cache

import numpy as np
import pytest

from tests import distinct_ref as R
from tests import exact_regimes as E
from tests import where_cases as W

pytestmark = pytest.mark.gpu

METRIC = {"ip": 0, "cosine": 1, "l2": 2}
NQ_MAX = 300


@pytest.fixture(scope="module")
def rmu():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import ragmeup_amd
    from ragmeup_amd import _native
    _native.lib()
    return ragmeup_amd


def _dpad(dim: int, metric: str) -> int:
    d = dim + 1 if metric == "l2" else dim
    return 192 if d <= 192 else (384 if d <= 384 else 768)


@lru_cache(maxsize=None)
def _base(dim: int, n: int):
    """(rows [n, dim] of norm 0.5 .. 1.5, unit queries [NQ_MAX, dim]), seeded"""
    rng = np.random.default_rng(1000 * dim + n)
    x = rng.standard_normal((n, dim), dtype=np.float32)
    x *= (rng.uniform(0.5, 1.5, (n, 1)) / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)
    q = rng.standard_normal((NQ_MAX, dim), dtype=np.float32)
    q /= np.linalg.norm(q, axis=1, keepdims=True).astype(np.float32)
    return np.ascontiguousarray(x, np.float32), np.ascontiguousarray(q, np.float32)


# ---- code layouts: (x, q, plan) -> (x', codes) ---------------------------------------------------------------------------------------------
def _flood_rows(p: dict, n: int, first_chunk: int, m: int = 200) -> np.ndarray:
    """m rows from chunk `first_chunk` on: a run across a workgroup-chunk boundary, a run across a tile boundary inside a chunk, a run of
    100 inside one chunk (more than CAP = 64 rows of one group in one slot), short runs across every 32-row row-part boundary of a tile,
    the rest every third row"""
    cr, rt = p["chunk_rows"], p["RT"]
    c0 = first_chunk * cr
    rows = [c0 + cr - 20 + np.arange(40)]                                           # chunk boundary (also a tile boundary)
    if p["tiles_per_chunk"] >= 2:
        rows.append(c0 + cr + rt - 15 + np.arange(30))                              # tile boundary inside chunk first_chunk + 1
    rows.append(c0 + 2 * cr + 3 + np.arange(min(100, cr - 6)))                      # deep in one chunk
    for b in range(32, rt, 32):
        rows.append(c0 + 3 * cr + b - 4 + np.arange(8))                             # row-part boundaries (WQ = 1: 128-row tiles)
    have = np.unique(np.concatenate(rows))
    rest = c0 + 4 * cr + 3 * np.arange(m)
    rows = np.unique(np.concatenate([have, rest[:max(0, m - have.size)]]))[:m]
    assert rows.size == m and rows[-1] < n, (rows.size, rows[-1], n)
    chunks = np.unique(rows // cr)
    assert chunks.size >= 4 and (np.bincount(rows // cr).max() > 64)
    return rows.astype(np.int64)


def lay_unique(x, q, p, arg):
    return x, np.arange(x.shape[0], dtype=np.int32)


def lay_one(x, q, p, arg):
    return x, np.full(x.shape[0], 7, np.int32)


def lay_mod(x, q, p, arg):
    return x, (np.arange(x.shape[0]) % arg).astype(np.int32)


def lay_flood(x, q, p, arg):
    """`arg` floods of 200 scaled copies of query 0 (and of queries 1, 2 ...: flood f serves query f too), each flood one group; their
    scales interleave, so the groups' order is decided by single rows.  The other rows: 50 groups behind them."""
    n = x.shape[0]
    x = x.copy()
    codes = (arg + np.arange(n) % 50).astype(np.int32)
    rng = np.random.default_rng(7)
    for f in range(arg):
        rows = _flood_rows(p, n, 1 + f, 200)
        # 1.0 .. 1.6, distinct over all floods, shuffled over the rows: above every other row's inner product (|x| <= 1.5, cosines below
        # 0.5) and, as squared distances (c - 1)^2 <= 0.36, below every other row's
        scale = (1.0 + (rng.permutation(200) * arg + f) / 1000.0).astype(np.float32)
        x[rows] = scale[:, None] * q[0][None, :]
        codes[rows] = f
    return x, codes


def lay_ties(x, q, p, arg):
    """bit-identical rows.  Query 1: two equal best rows in ONE group (the lower id represents), then two equal rows in DIFFERENT groups (the
    lower id's group first).  Query 2: arg + 1 equal rows in arg + 1 groups, one per workgroup chunk -- a tie exactly at rank k = arg"""
    n, cr = x.shape[0], p["chunk_rows"]
    x = x.copy()
    codes = (100 + np.arange(n) % 97).astype(np.int32)
    a, b, c, d = cr + 5, 3 * cr + 1, 2 * cr - 1, 2 * cr
    x[[a, b]] = np.float32(3.0) * q[1]
    codes[[a, b]] = 1
    x[[c, d]] = np.float32(2.5) * q[1]
    codes[[c, d]] = [2, 3]
    rows = 7 + (cr + 1) * np.arange(arg + 1)
    rows = rows[rows < n]
    if rows.size < arg + 1:                                  # a small corpus: next to each other
        rows = n - 2 - arg + np.arange(arg + 1)
    x[rows] = np.float32(3.0) * q[2]
    codes[rows] = 10 + np.arange(arg + 1)
    return x, codes


@dataclass(frozen=True)
class Case:
    dim: int
    metric: str
    n: int
    nq: int
    k: int
    lay: str
    arg: int = 0

    @property
    def id(self):
        return f"{self.metric}-d{self.dim}-n{self.n}-nq{self.nq}-k{self.k}-{self.lay}{self.arg or ''}"


LAY = {"unique": lay_unique, "one": lay_one, "mod": lay_mod, "flood": lay_flood, "ties": lay_ties}

# rows per geometry that give a workgroup three tiles: WQ = 1 (nq <= 32): 256 chunks of 128-row tiles; WQ = 4: 256 (128 with two query
# tiles) chunks of 32-row tiles
N_W1, N_W4 = 513 * 128 + 1, 513 * 32 + 1

CASES = (
    # one row per group == FlatIndex.search, in both geometries, three widths, three metrics
    [Case(100, "ip", n, nq, 10, "unique") for n in (1, 127, 128, 129) for nq in (1, 33)]
    + [Case(100, "ip", N_W1, 32, 10, "unique"), Case(100, "ip", N_W4, 33, 32, "unique"), Case(384, "cosine", N_W4, 129, 10, "unique"),
       Case(384, "ip", N_W4, 300, 1, "unique"), Case(768, "ip", 4099, 1, 32, "unique"), Case(767, "l2", 4099, 33, 10, "unique"),
       Case(383, "l2", 8200, 32, 10, "unique")]
    # one group for the whole corpus: one hit, then padding
    + [Case(100, "ip", 2000, 1, 10, "one"), Case(384, "cosine", 2000, 33, 32, "one"), Case(100, "l2", 129, 32, 1, "one")]
    # code = row % G around k
    + [Case(100, "ip", 5000, nq, 10, "mod", g) for nq in (1, 129) for g in (9, 10, 11, 1000)]
    + [Case(384, "l2", 5000, 32, 32, "mod", g) for g in (31, 32, 33)] + [Case(768, "cosine", 3000, 33, 1, "mod", 2)]
    # floods: the 200 best rows in one group; three floods in three groups
    + [Case(100, "ip", N_W1, 32, 10, "flood", 1), Case(100, "ip", N_W1, 1, 10, "flood", 3), Case(384, "ip", N_W4, 33, 10, "flood", 1),
       Case(384, "cosine", N_W4, 129, 32, "flood", 3), Case(383, "l2", N_W4, 300, 10, "flood", 3), Case(768, "ip", N_W4, 33, 1, "flood", 1)]
    # bit-identical rows
    + [Case(100, "ip", N_W4, 32, 10, "ties", 10), Case(384, "ip", N_W4, 33, 10, "ties", 10), Case(100, "cosine", 5000, 129, 32, "ties", 32),
       Case(100, "ip", 129, 33, 1, "ties", 1)]
)


@lru_cache(maxsize=4)
def _world(c: Case):
    x, q = _base(c.dim, c.n)
    q = q[:c.nq]
    x, codes = LAY[c.lay](x, q, R.plan(c.n, c.nq), c.arg)
    scores, qn2 = R.chain_scores(c.metric, q, x, c.dim, _dpad(c.dim, c.metric))
    return x, q, codes, scores, qn2


def _open(rmu, dim, metric, x, codes):
    idx = rmu.FlatIndex(dim, metric=METRIC[metric])
    idx.set_screening(False)
    cols = rmu.Columns(1)
    half = x.shape[0] // 2
    for lo, hi in ((0, half), (half, x.shape[0])):            # two appends: the tail upload of the image
        if hi > lo:
            idx.add(x[lo:hi])
            cols.append(np.ascontiguousarray(codes[lo:hi, None], np.int32))
    return idx, cols


@pytest.mark.parametrize("c", CASES, ids=lambda c: c.id)
def test_search_distinct_equals_the_reference(rmu, c):
    x, q, codes, scores, qn2 = _world(c)
    want = R.distinct_from_scores(scores, None, codes, c.k, qn2)
    if c.lay == "flood":                                       # the construction holds: the 200 best rows of query 0 carry one code
        top = E.ranked(scores[:1], None, 200)[1][0]
        assert (codes[top] < c.arg).all() and (c.arg > 1 or (codes[top] == 0).all())
        assert len(set(codes[want[1][0, :c.arg]])) == min(c.arg, c.k) and (want[1][0] >= 0).sum() == min(c.k, 50 + c.arg)
    if c.lay == "one":
        assert (want[1][:, 0] >= 0).all() and (want[1][:, 1:] == -1).all()
    if c.lay == "mod" and c.arg < c.k:
        assert ((want[1] >= 0).sum(axis=1) == min(c.arg, c.n)).all()
    idx, cols = _open(rmu, c.dim, c.metric, x, codes)
    got = idx.search_distinct(q, c.k, cols, 0)
    g = idx.last_geometry()
    p = R.plan(c.n, c.nq)
    assert g["grid"] == p["grid"], (g, p)
    m = E.mismatch(*got, *want)
    assert not m, f"{c.id}: {m}"
    if c.lay == "unique":                                      # one row per group: the established kernel's answer, bit for bit
        m = E.mismatch(*got, *idx.search(q, c.k))
        assert not m, f"{c.id} against FlatIndex.search: {m}"
    if c.lay == "ties":
        r = got[1]
        if c.nq > 2 and c.arg > 1:
            a, cc, d = p["chunk_rows"] + 5, 2 * p["chunk_rows"] - 1, 2 * p["chunk_rows"]
            if c.metric == "ip":                               # (normalised, 3 q and 2.5 q need not be the same bits: the reference decides)
                assert r[1, 0] == a and (c.k < 3 or (r[1, 1] == cc and r[1, 2] == d))
            tied = np.nonzero(codes[:, None] == (10 + np.arange(c.arg + 1))[None, :])[0]
            assert tied.size == c.arg + 1 and r[2].tolist() == sorted(tied.tolist())[:c.k]
    idx.close(); cols.close()


def test_deletes_then_compaction(rmu):
    dim, n, k = 100, 5000, 10
    x, q = _base(dim, n)
    codes = (np.arange(n) % 40).astype(np.int32)
    for metric, nq in (("ip", 33), ("l2", 4)):
        qq = q[:nq]
        scores, qn2 = R.chain_scores(metric, qq, x, dim, _dpad(dim, metric))
        idx, cols = _open(rmu, dim, metric, x, codes)
        alive = np.ones(n, bool)
        check = lambda what: (lambda m: m == "" or pytest.fail(f"{metric} {what}: {m}"))(
            E.mismatch(*idx.search_distinct(qq, k, cols, 0), *R.distinct_from_scores(scores, alive, codes, k, qn2)))
        check("before")
        # the representatives of the best groups of every query: the next best row of each group takes over
        reps = np.unique(idx.search_distinct(qq, k, cols, 0)[1])
        reps = reps[reps >= 0]
        assert idx.remove_rows(reps) == reps.size
        alive[reps] = False
        check("representatives removed")
        # a whole group
        gone = np.nonzero(codes == 3)[0]
        idx.remove_rows(gone[alive[gone]])
        alive[gone] = False
        got = idx.search_distinct(qq, k, cols, 0)
        assert not np.isin(got[1][got[1] >= 0], gone).any()
        check("a group removed")
        # compact the index and the columns: the same answer with the ids mapped
        before = idx.search_distinct(qq, k, cols, 0)
        o2n = idx.compact()
        assert cols.compact(o2n) == len(idx) == int(alive.sum())
        after = idx.search_distinct(qq, k, cols, 0)
        mapped = np.where(before[1] >= 0, np.asarray(o2n)[np.maximum(before[1], 0)], -1)
        m = E.mismatch(after[0], after[1], before[0], mapped)
        assert not m, f"{metric} after compaction: {m}"
        # everything removed: all padding
        idx.remove_rows(np.arange(len(idx)))
        s, r = idx.search_distinct(qq, k, cols, 0)
        assert (r == -1).all() and (np.isposinf(s) if metric == "l2" else np.isneginf(s)).all()
        idx.close(); cols.close()
    # an empty index and empty columns
    idx, cols = rmu.FlatIndex(dim), rmu.Columns(1)
    s, r = idx.search_distinct(q[:3], 5, cols, 0)
    assert (r == -1).all() and np.isneginf(s).all()
    idx.close(); cols.close()


def test_device_queries_a_caller_stream_row_base_and_more_than_one_field(rmu):
    import torch
    from ragmeup_amd import _native as N
    dim, n, nq, k = 100, 3000, 40, 10
    x, q = _base(dim, n)
    q = q[:nq]
    codes = np.stack([np.arange(n) % 3, np.arange(n) % 25, np.arange(n) // 100], axis=1).astype(np.int32)
    idx = rmu.FlatIndex(dim)
    idx.add(x)
    cols = rmu.Columns(3)
    cols.append(codes)
    scores, _ = R.chain_scores("ip", q, x, dim, 192)
    for field in range(3):
        want = R.distinct_from_scores(scores, None, codes[:, field], k, row_base=10_000)
        m = E.mismatch(*idx.search_distinct(q, k, cols, field, row_base=10_000), *want)
        assert not m, f"host, field {field}: {m}"
        ds, dr = idx.search_distinct(torch.from_numpy(q).cuda(), k, cols, field, row_base=10_000)
        assert ds.is_cuda and dr.is_cuda and dr.dtype == torch.int64
        m = E.mismatch(ds.cpu().numpy(), dr.cpu().numpy(), *want)
        assert not m, f"device, field {field}: {m}"
    # a caller stream, device queries and outputs, straight through the C ABI
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        qd = torch.from_numpy(q).cuda()
        out_s = torch.empty((nq, k), dtype=torch.float32, device="cuda")
        out_r = torch.empty((nq, k), dtype=torch.int64, device="cuda")
        N.check(N.lib().rmu_index_search_distinct(idx._h, cols._h, 1, qd.data_ptr(), nq, k, N.F_Q_DEVICE | N.F_OUT_DEVICE, 0, out_s.data_ptr(),
                                                  out_r.data_ptr(), st.cuda_stream), "rmu_index_search_distinct")
    st.synchronize()
    m = E.mismatch(out_s.cpu().numpy(), out_r.cpu().numpy(), *R.distinct_from_scores(scores, None, codes[:, 1], k))
    assert not m, f"caller stream: {m}"
    idx.close(); cols.close()


def test_more_queries_than_one_block(rmu):
    from ragmeup_amd import _native as N
    dim, n, k = 64, 300, 5
    x, q = _base(dim, n)
    nq = N.MAX_QUERIES_PER_CALL + 5
    qq = np.ascontiguousarray(np.tile(q, (nq // NQ_MAX + 1, 1))[:nq] * np.linspace(0.5, 1.5, nq, dtype=np.float32)[:, None])
    codes = (np.arange(n) % 7).astype(np.int32)
    idx, cols = _open(rmu, dim, "ip", x, codes)
    m = E.mismatch(*idx.search_distinct(qq, k, cols, 0), *R.search_distinct("ip", qq, x, codes, k, dim, 192))
    assert not m, m
    idx.close(); cols.close()


def test_refusals(rmu):
    from ragmeup_amd import _native as N
    lib = N.lib()
    wide = rmu.FlatIndex(1024)
    wide.add(np.ones((4, 1024), np.float32))
    cols = rmu.Columns(1)
    cols.append(np.zeros((4, 1), np.int32))
    q = np.zeros((1, 1024), np.float32)
    with pytest.raises(ValueError):
        wide.search_distinct(q, 2, cols, 0)
    s, r = np.zeros((1, 2), np.float32), np.zeros((1, 2), np.int64)
    with pytest.raises(N.RmuError, match="wide index") as e:
        N.check(lib.rmu_index_search_distinct(wide._h, cols._h, 0, q.ctypes.data, 1, 2, 0, 0, s.ctypes.data, r.ctypes.data, 0), "rmu_index_search_distinct")
    assert e.value.code == -1
    wide.close(); cols.close()
    # columns one row short
    idx = rmu.FlatIndex(64)
    idx.add(_base(64, 50)[0])
    cols = rmu.Columns(1)
    cols.append(np.zeros((49, 1), np.int32))
    with pytest.raises(N.RmuError, match="out of step") as e:
        idx.search_distinct(_base(64, 50)[1][:2], 3, cols, 0)
    assert e.value.code == -1
    cols.append(np.zeros((1, 1), np.int32))                   # in step again: served
    assert idx.search_distinct(_base(64, 50)[1][:2], 3, cols, 0)[1][:, 1:].tolist() == [[-1, -1], [-1, -1]]
    with pytest.raises(N.RmuError):
        idx.search_distinct(_base(64, 50)[1][:2], 33, cols, 0)
    idx.close(); cols.close()


# ---- the store, end to end ----------------------------------------------------------------------------------------------------------------
def _expected_docs(st, emb, queries, k):
    """one (text, source) per source and query, in the reference's order, from the records the store holds"""
    x = np.asarray(emb.embed_documents(st._texts), np.float32)
    q = np.asarray(emb.embed_documents(queries), np.float32)
    vals = {}
    codes = np.array([vals.setdefault(m.get("source"), len(vals)) for m in st._metas], np.int32)
    _, rows = R.search_distinct("ip", q, x, codes, k, emb.dim, 192, alive=np.asarray(st._alive, bool))
    return [[(st._texts[r], st._metas[r]["source"]) for r in rr if r >= 0] for rr in rows]


def test_the_store_returns_one_document_per_source(rmu):
    from ragmeup_amd.vectorstore import MI355XVectorStore
    emb = W.HashEmbeddings(96)
    n = 600
    texts = ["chunk %d of the corpus" % i for i in range(n)]
    metas = [{"source": "doc%02d.pdf" % (i // 40), "page": i % 40} for i in range(n)]
    ids = ["pk%04d" % i for i in range(n)]
    st = MI355XVectorStore(embeddings=emb, collection_name="distinct-gpu", auto_persist=False, device_fields=("source",))
    st.add_texts(texts[:400], metas[:400], ids=ids[:400])
    queries = [texts[5], texts[45], texts[399], "something else entirely"]
    rt = st.as_retriever(search_kwargs={"k": 4, "group_by": "source"})

    def check(what):
        want = _expected_docs(st, emb, queries, 4)
        for qi, query in enumerate(queries):
            got = st.similarity_search(query, k=4, group_by="source")
            assert [(d.page_content, d.metadata["source"]) for d in got] == want[qi], (what, qi)
            assert len({d.metadata["source"] for d in got}) == len(got) == 4
            assert [(d.page_content, d.metadata["source"]) for d in rt.invoke(query)] == want[qi], (what, qi)
        batch = rt.batch_invoke(queries)
        assert [[(d.page_content, d.metadata["source"]) for d in row] for row in batch] == want, what
        return want
    w0 = check("first upload")
    assert w0[0][0][0] == texts[5] and w0[1][0][0] == texts[45]
    plain = st.similarity_search(texts[5], k=4)                 # without group_by the chunks of one source may repeat; the scores agree
    scored = dict((d.page_content, s) for d, s in st.similarity_search_with_score(texts[5], k=4))
    for d, s in st.similarity_search_with_score(texts[5], k=4, group_by="source"):
        if d.page_content in scored:
            assert s == scored[d.page_content]
    assert plain[0].page_content == texts[5]
    st.add_texts(texts[400:], metas[400:], ids=ids[400:])       # an upload
    assert len(st._columns) == len(st._index) == n
    check("second upload")
    st.delete(ids=[ids[5], ids[45]])                            # the representatives of two sources ...
    st.delete(expr='source == "doc09.pdf"')                     # ... and a whole source
    w2 = check("deleted")
    assert all(src != "doc09.pdf" for row in w2 for _, src in row) and w2[0][0][0] != texts[5]
    assert st.compact() > 0 and len(st._columns) == len(st._index)
    assert check("compacted") == w2
    with pytest.raises(ValueError, match="device_fields="):
        st.similarity_search(texts[5], k=4, group_by="page")
