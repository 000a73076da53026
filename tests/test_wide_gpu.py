"""GPU tests of the wide flat index (rows of 769..3072 dimensions, scan_wide.hip) against the fp64 oracle, and of scan_wide_kernel against
scan_topk_kernel, bit for bit, at the widths both serve (RMU_OPT_WIDE_SCAN): the index's life cycle, its limits and the store on top.

The bit-level bar of the kernel itself lives in tests/test_wide_regimes_gpu.py (cases: tests/wide_regimes.py): every configuration,
tile class, block-map branch and query-tile count against the fmaf chain, with no tolerance and no tie rule, on corpora that fill the
candidate slots.  The ladder test below is held to the same chain.

Bar here: tests.helpers.assert_topk_parity with its default tolerances against oracle.flat_search run 4 deeper than k, and at most 1% of the
returned positions forgiven as near-ties (neighbouring fp64 scores closer than 1e-6 are 0.4-0.9% of the top 116 of 5000 unit-norm
Gaussian rows at widths 769..3072; a plain fp32 product is within 1.1e-7 of fp64).
"""
import functools
import hashlib
import os

import numpy as np
import pytest

from oracle import oracle as O
from tests.helpers import assert_topk_parity

pytestmark = pytest.mark.gpu

IP, COSINE, L2SQ = 0, 1, 2


@pytest.fixture(scope="module")
def rmu():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import ragmeup_amd
    from ragmeup_amd import _native
    _native.lib()
    return ragmeup_amd


@functools.lru_cache(maxsize=4)
def _data(n, dim, metric, seed=1):
    """Unit-norm Gaussian rows and queries; cosine: rows and queries rescaled by 0.2..5 (the index normalises).  Read-only."""
    x = O.make_corpus(n, dim, seed=seed)
    q = O.make_corpus(130, dim, seed=seed + 100)
    if metric == COSINE:
        rng = np.random.default_rng(seed + 200)
        x = x * rng.uniform(0.2, 5.0, (n, 1)).astype(np.float32)
        q = q * rng.uniform(0.2, 5.0, (130, 1)).astype(np.float32)
    x.setflags(write=False)
    q.setflags(write=False)
    return x, q


def _check(s, r, q, x, k, metric, alive=None, block=262144):
    """parity with the oracle, 4 deeper than k; returns (forgiven positions, positions)"""
    n_live = x.shape[0] if alive is None else int(alive.sum())
    os_, or_ = O.flat_search(q, x, k + 4, metric=metric, alive=alive, block=block)
    assert_topk_parity(s, r, os_, or_)
    forgiven = int((r != or_[:, :k]).sum())
    assert forgiven <= 0.01 * r.size, (forgiven, r.size)
    if n_live < k:
        assert (r[:, n_live:] == -1).all() and np.isneginf(s[:, n_live:]).all()
    return forgiven, r.size


# every width, every query geometry (<= 32, <= 64, more; both sides of each switch), both candidate-slot classes (k <= 32, k <= 112)
GRID = [(769, IP, 1, 10), (769, COSINE, 130, 33), (769, IP, 64, 32),
        (1024, IP, 33, 10), (1024, COSINE, 64, 32), (1024, IP, 65, 1), (1024, IP, 130, 112), (1024, COSINE, 1, 33),
        (1536, COSINE, 1, 10), (1536, IP, 130, 10), (1536, IP, 64, 112), (1536, COSINE, 65, 33),
        (3072, IP, 130, 10), (3072, COSINE, 33, 112), (3072, IP, 1, 1), (3072, IP, 65, 32)]


@pytest.mark.parametrize("dim,metric,nq,k", GRID)
def test_parity_grid(rmu, dim, metric, nq, k):
    x, q = _data(5000, dim, metric)
    idx = rmu.FlatIndex(dim, metric=metric)
    idx.add(x)
    s, r = idx.search(q[:nq], k)
    print("forgiven / positions:", _check(s, r, q[:nq], x, k, metric))
    assert (np.diff(s, axis=1) <= 0).all()
    idx.close()


@pytest.mark.parametrize("n", [0, 1, 31, 129])
def test_fewer_live_rows_than_k_and_the_empty_index(rmu, n):
    x = O.make_corpus(n, 1024, seed=5) if n else np.zeros((0, 1024), np.float32)
    q = O.make_corpus(5, 1024, seed=6)
    idx = rmu.FlatIndex(1024)
    if n:
        idx.add(x)
    for k in (1, 10, 40):
        s, r = idx.search(q, k)
        _check(s, r, q, x, k, IP)
        assert (r[:, n:] == -1).all() and np.isneginf(s[:, n:]).all()
    idx.close()


def test_equal_scores_come_back_lowest_row_first(rmu):
    x = O.make_corpus(600, 1024, seed=7).copy()
    x[300] = x[100]
    x[500] = x[100]
    idx = rmu.FlatIndex(1024)
    idx.add(x)
    for k in (3, 10, 40):
        s, r = idx.search(x[100:101], k)
        assert r[0, :3].tolist() == [100, 300, 500]
        assert len(set(s[0, :3].view(np.int32).tolist())) == 1
    idx.close()


def test_score_bits_do_not_depend_on_batch_k_or_allocation(rmu):
    x, q = _data(3000, 1536, IP, seed=3)
    idx = rmu.FlatIndex(1536)
    idx.add(x)
    s1, r1 = idx.search(q[:1], 10)
    runs = {"batch 33": idx.search(q[:33], 10), "batch 130": idx.search(q[:130], 10), "k 40": idx.search(q[:1], 40)}
    idx.reserve(3000 * 4)                                   # a re-allocation: rows move to another matrix
    assert idx.stats()["grow_count"] >= 1
    runs["after reserve"] = idx.search(q[:1], 10)
    for name, (s, r) in runs.items():
        assert np.array_equal(r[0, :10], r1[0]), name
        assert np.array_equal(s[0, :10].view(np.int32), s1[0].view(np.int32)), name
    idx.close()


@pytest.mark.parametrize("metric", [IP, COSINE])
@pytest.mark.parametrize("dim", [100, 384, 768])
def test_the_wide_kernel_returns_the_established_kernels_bits(rmu, dim, metric):
    x, q = _data(20000, dim, metric, seed=9)
    idx = rmu.FlatIndex(dim, metric=metric)
    idx.add(x)
    idx.set_screening(False)
    for nq in (1, 40, 130):
        for k in (10, 40):
            idx.set_wide_scan(False)
            s0, r0 = idx.search(q[:nq], k)
            g0 = idx.last_geometry()
            idx.set_wide_scan(True)
            s1, r1 = idx.search(q[:nq], k)
            g1 = idx.last_geometry()
            assert np.array_equal(r0, r1), (nq, k)
            assert np.array_equal(s0.view(np.int32), s1.view(np.int32)), (nq, k)
            assert g0 != g1, (nq, k, g0)                     # the other kernel ran
    idx.set_wide_scan(False)
    idx.close()


def test_wide_scan_option_is_refused_on_an_l2_index(rmu):
    from ragmeup_amd import _native as N
    idx = rmu.FlatIndex(64, metric=L2SQ)
    with pytest.raises(N.RmuError) as e:
        idx.set_wide_scan(True)
    assert e.value.code == -1
    idx.close()


_LADDER_CHILD = """
import sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from tests.test_wide_gpu import _ladder_data
from ragmeup_amd import FlatIndex
x, q = _ladder_data()
idx = FlatIndex(1024, capacity_hint=x.shape[0])
idx.add(x)
s, r = idx.search(q, 40)
np.savez(sys.argv[2], s=s, r=r, launches=idx.last_geometry()["launches"])
"""


def _ladder_data():
    n = 262144 + 77
    rng = np.random.default_rng(11)
    x = rng.standard_normal((n, 1024), dtype=np.float32)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    return x, O.make_corpus(8, 1024, seed=12)


def test_exact_ladder_over_a_large_corpus(rmu, tmp_path):
    """k > 32 over >= 262 144 rows: the exact threshold ladder, every launch the wide kernel with a row0 and seeded shared thresholds.
    The ladder's geometry (RMU_DEEP_FIRST / RMU_DEEP_RATIO, read once per process under RMU_TUNING=1: a child process) and the
    per-index ladder options change nothing in the result."""
    import subprocess
    import sys
    x, q = _ladder_data()
    env = dict(os.environ, RMU_TUNING="1", RMU_DEEP_FIRST="2048", RMU_DEEP_RATIO="2")
    out = str(tmp_path / "child.npz")
    child = subprocess.Popen([sys.executable, "-c", _LADDER_CHILD, os.path.dirname(os.path.dirname(os.path.abspath(__file__))), out], env=env)
    idx = rmu.FlatIndex(1024, capacity_hint=x.shape[0])
    idx.add(x)
    s, r = idx.search(q, 40)
    launches = idx.last_geometry()["launches"]
    assert launches > 1
    print("forgiven / positions:", _check(s, r, q, x, 40, IP, block=32768))
    from tests import exact_regimes as E
    assert not E.mismatch(s, r, *E.expected_topk(E.chain(q, x, 1024), None, 40))      # ... and to the fmaf chain, bit for bit
    for ratio, first in ((8, 256), (3, 16384)):              # accepted, no effect
        idx.set_ladder(ratio, first)
        s2, r2 = idx.search(q, 40)
        assert np.array_equal(r2, r) and np.array_equal(s2.view(np.int32), s.view(np.int32))
    idx.set_ladder(0, 0)
    assert child.wait(timeout=120) == 0
    got = np.load(out)
    assert int(got["launches"]) != launches                  # another ladder ...
    assert np.array_equal(got["r"], r) and np.array_equal(got["s"].view(np.int32), s.view(np.int32))    # ... the same bits
    idx.set_screening(False)                                 # accepted, no effect
    idx.set_screen_min_batch(1)
    s3, r3 = idx.search(q, 40)
    assert idx.last_screened() == 0
    assert np.array_equal(r3, r) and np.array_equal(s3.view(np.int32), s.view(np.int32))
    idx.close()


@pytest.mark.parametrize("metric", [IP, COSINE])
def test_lifecycle_at_width_1024(rmu, metric, tmp_path):
    import torch
    n, dim, k = 6000, 1024, 10
    x, q = _data(n, dim, metric, seed=13)
    q = q[:40]
    idx = rmu.FlatIndex(dim, metric=metric)                  # default capacity 4096: the second add crosses a growth
    assert idx.add(x[:700]) == 0 and idx.add(x[700:4500]) == 700 and idx.add(x[4500:]) == 4500
    assert idx.stats()["grow_count"] >= 1 and len(idx) == n
    alive = np.ones(n, bool)
    dead = np.random.default_rng(14).choice(n, n // 10, replace=False)
    alive[dead] = False
    assert idx.remove_rows(dead) == n // 10
    s, r = idx.search(q, k)
    _check(s, r, q, x, k, metric, alive=alive)
    stored = x / np.linalg.norm(x, axis=1, keepdims=True) if metric == COSINE else x
    live = np.nonzero(alive)[0]
    for inplace in (False, True):
        other = rmu.FlatIndex(dim, metric=metric)
        other.add(x)
        other.remove_rows(dead)
        if inplace:
            other.set_compact_inplace(True)
        m = other.compact()
        assert len(other) == live.size and m.shape == (n,)
        assert np.array_equal(m[live], np.arange(live.size)) and (m[dead] == -1).all()
        s2, r2 = other.search(q, k)
        _check(s2, r2, q, x[live], k, metric)
        assert np.array_equal(r2, m[r]) and np.array_equal(s2.view(np.int32), s.view(np.int32))
        got = other.get_rows(np.array([0, 1, live.size - 1]))
        assert np.abs(got - stored[live[[0, 1, -1]]]).max() <= 1e-6
        if not inplace:
            p = str(tmp_path / "wide.rmu")
            other.save(p)
            back = rmu.FlatIndex.load(p)
            assert back.dim == dim and back.metric == metric and len(back) == live.size
            s3, r3 = back.search(q, k)
            assert np.array_equal(r3, r2) and np.array_equal(s3.view(np.int32), s2.view(np.int32))
            back.close()
            # search_mmr == search + mmr
            rows_m, sc_m = other.search_mmr(q[:6], fetch_k=20, k=5)
            s20, r20 = other.search(q[:6], 20)
            pos = other.mmr(q[:6], r20, 5)
            assert np.array_equal(rows_m, np.take_along_axis(r20, pos.astype(np.int64), axis=1))
            assert np.array_equal(sc_m.view(np.int32), np.take_along_axis(s20, pos.astype(np.int64), axis=1).view(np.int32))
            # device queries and outputs on a caller stream == the host path
            st = torch.cuda.Stream()
            with torch.cuda.stream(st):
                qd = torch.from_numpy(q.copy()).cuda()
                out = (torch.empty((q.shape[0], k), dtype=torch.float32, device="cuda"), torch.empty((q.shape[0], k), dtype=torch.int64, device="cuda"))
                st.synchronize()
                sd, rd = other.search(qd, k, row_base=1000, stream=st.cuda_stream, out=out)
                st.synchronize()
            assert np.array_equal(rd.cpu().numpy(), np.where(r2 >= 0, r2 + 1000, r2))
            assert np.array_equal(sd.cpu().numpy().view(np.int32), s2.view(np.int32))
        other.close()
    idx.close()


class Stub1024:
    """A foreign Embeddings object: seeded 1024-d unit vectors, no encoder, no fused query path."""
    dim = 1024

    def _vec(self, text):
        seed = int.from_bytes(hashlib.sha256(text.encode()).digest()[:8], "little")
        v = np.random.default_rng(seed).standard_normal(self.dim)
        return (v / np.linalg.norm(v)).astype(np.float32)

    def embed_documents(self, texts):
        return [self._vec(t).tolist() for t in texts]

    def embed_query(self, text):
        v = self._vec("doc %d" % (int(hashlib.md5(text.encode()).hexdigest(), 16) % 300)) + 0.3 * self._vec("noise " + text)
        return (v / np.linalg.norm(v)).astype(np.float32).tolist()


def test_declared_limits(rmu):
    from ragmeup_amd import _native as N
    from ragmeup_amd.vectorstore import MI355XVectorStore
    idx = rmu.FlatIndex(1024)
    idx.add(O.make_corpus(200, 1024, seed=15))
    with pytest.raises(ValueError, match="768"):
        idx.search(O.make_corpus(2, 1024, seed=16), 5, rows=np.arange(0, 100, dtype=np.int64))
    # ... and the C entry point itself refuses before anything is enqueued
    qq, rr = O.make_corpus(2, 1024, seed=16), np.arange(0, 100, dtype=np.int64)
    os_, or_ = np.empty((2, 5), np.float32), np.empty((2, 5), np.int64)
    rc = N.lib().rmu_index_search_subset(idx._h, qq.ctypes.data, 2, 5, 0, 0, rr.ctypes.data, 100, os_.ctypes.data, or_.ctypes.data, 0)
    assert rc == -1 and b"768" in N.lib().rmu_last_error()
    idx.close()
    with pytest.raises(N.RmuError, match="L2"):
        rmu.FlatIndex(1024, metric=L2SQ)
    with pytest.raises(N.RmuError, match="3072"):
        rmu.FlatIndex(3073)
    st = MI355XVectorStore(embeddings=Stub1024(), collection_name="wide-limits", auto_persist=False)
    st.add_texts(["doc %d" % i for i in range(50)], [{"source": "a.pdf"}] * 50)
    assert len(st.similarity_search("a wave", k=3)) == 3
    with pytest.raises(ValueError, match="768"):
        st.similarity_search("a wave", k=3, expr='source == "a.pdf"')
    with pytest.raises(ValueError, match="768"):
        st.max_marginal_relevance_search("a wave", k=3, filter={"source": "a.pdf"})


def test_store_end_to_end_with_foreign_1024d_embeddings(rmu, tmp_path):
    from ragmeup_amd.vectorstore import MI355XVectorStore
    emb = Stub1024()
    texts = ["doc %d" % i for i in range(300)]
    metas = [{"source": "%s.pdf" % "abc"[i % 3]} for i in range(300)]
    ids = ["pk%03d" % i for i in range(300)]
    uri = str(tmp_path / "wide.db")
    st = MI355XVectorStore.from_texts(texts, emb, metadatas=metas, ids=ids, connection_args={"uri": uri}, collection_name="wide",
                                      auto_persist=False, drop_old=True)

    def ranking(query, live_texts, k):
        v = np.array([emb._vec(t) for t in live_texts], np.float64)
        sc = v @ np.asarray(emb.embed_query(query), np.float64)
        order = np.argsort(-sc, kind="stable")[:k]
        return [live_texts[i] for i in order], sc[order]

    queries = ["what is a wave", "lane and tile", "hbm bandwidth"]
    for query in queries:
        hits = st.similarity_search_with_score(query, k=6)
        want, sc = ranking(query, texts, 6)
        assert [d.page_content for d, _ in hits] == want
        assert np.abs(np.array([s for _, s in hits]) - (2.0 - 2.0 * sc)).max() <= 1e-4      # ip on unit vectors reports Milvus "L2"
        mm = st.max_marginal_relevance_search(query, k=4, fetch_k=20)
        cand, _ = ranking(query, texts, 20)
        cv = np.array([emb._vec(t) for t in cand], np.float32)
        picks = O.mmr(np.asarray(emb.embed_query(query), np.float32), cv, k=4, lambda_mult=0.5)
        assert [d.page_content for d in mm] == [cand[i] for i in picks]
    # upsert by id: the record's text (and vector) is replaced
    st.add_texts(["doc 7 rewritten"], [{"source": "z.pdf"}], ids=["pk007"])
    # delete by expression
    st.delete(expr='source == "b.pdf"')
    live = [("doc 7 rewritten" if i == 7 else t) for i, t in enumerate(texts) if metas[i]["source"] != "b.pdf" or i == 7]
    assert st.compact() > 0
    before = {}
    for query in queries:
        hits = st.similarity_search_with_score(query, k=6)
        want, _ = ranking(query, live, 6)
        assert sorted(d.page_content for d, _ in hits) == sorted(want) and [d.page_content for d, _ in hits] == want
        before[query] = [(d.page_content, s) for d, s in hits]
    assert st.persist()
    again = MI355XVectorStore(embeddings=emb, collection_name="wide", connection_args={"uri": uri}, auto_persist=False)
    assert again.load()
    for query in queries:
        assert [(d.page_content, s) for d, s in again.similarity_search_with_score(query, k=6)] == before[query]
