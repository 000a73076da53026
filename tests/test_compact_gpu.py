"""GPU: rmu_index_compact -- dropping tombstoned rows leaves every search as it was (ids mapped through old_to_new, scores bit for bit),
on both storage paths (fresh allocations / in place), for every metric, on the screening and the exact path; the vacated tail is what a
fresh index holds there; the vector store reclaims the rows of a delete / re-upload cycle while searches run beside it."""
import ctypes
import hashlib
import os
import tempfile
import threading
import time

import numpy as np
import pytest

from oracle import oracle as O
from tests.helpers import assert_topk_parity

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rmu():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import ragmeup_amd
    from ragmeup_amd import _native
    _native.lib()
    return ragmeup_amd


def _metric(name):
    from ragmeup_amd import _native as N
    return {"ip": N.METRIC_IP, "cosine": N.METRIC_COSINE, "l2": N.METRIC_L2SQ}[name]


def _dead_rows(n, rng, frac=0.3):
    dead = set(rng.choice(n, int(frac * n), replace=False).tolist())
    dead |= set(range(n // 3, n // 3 + 1500))                  # a contiguous block
    dead |= {0, n - 1}
    return np.array(sorted(dead), np.int64)


def _mapped(r, m):
    return np.where(r >= 0, m[np.maximum(r, 0)], -1)


def _set_path(idx, path):
    if path == "screen":
        idx.set_screen_min_batch(1)
    else:
        idx.set_screening(False)


def _oracle_parity(s, r, q, x_live, k, metric):
    from ragmeup_amd import _native as N
    os_, or_ = O.flat_search(q, x_live, k + 4, metric=metric)
    if metric == N.METRIC_L2SQ:
        scale = float(np.abs(os_[np.isfinite(os_)]).max(initial=1.0))
        assert_topk_parity(-s, r, os_, or_, score_tol=2e-6 * scale + 1e-4, tie_tol=1e-6 * scale)
    else:
        assert_topk_parity(s, r, os_, or_)


@pytest.fixture(scope="module")
def corpus():
    x = O.make_corpus(50_000)
    q, _ = O.make_queries(x, 64)
    rng = np.random.default_rng(3)
    xl2 = (x * rng.uniform(0.3, 3.0, (x.shape[0], 1))).astype(np.float32)      # un-normalised rows for the native L2 metric
    return x, xl2, q


@pytest.mark.parametrize("path", ["screen", "exact"])
@pytest.mark.parametrize("metric", ["ip", "cosine", "l2"])
def test_searches_after_compaction_equal_those_before(rmu, corpus, metric, path):
    x, xl2, q = corpus
    m_ = _metric(metric)
    xs = xl2 if metric == "l2" else x
    idx = rmu.FlatIndex(384, metric=m_)
    idx.add(xs[:20_000]); idx.add(xs[20_000:])
    _set_path(idx, path)
    dead = _dead_rows(len(xs), np.random.default_rng(7))
    assert idx.remove_rows(dead) == dead.size
    before = {k: idx.search(q, k) for k in (10, 100)}
    cap0 = idx.stats()["capacity"]
    m = idx.compact()
    live = np.setdiff1d(np.arange(len(xs)), dead)
    assert m.shape == (len(xs),) and (m[dead] == -1).all() and (m[live] == np.arange(live.size)).all()
    assert len(idx) == live.size and idx.stats()["live_rows"] == live.size and idx.stats()["capacity"] < cap0
    for k, (s0, r0) in before.items():
        s1, r1 = idx.search(q, k)
        assert np.array_equal(r1, _mapped(r0, m)), k
        assert np.array_equal(s1, s0), k
        _oracle_parity(s1, r1, q, xs[live], k, m_)
    if path == "screen":
        idx.search(q, 10)
        assert idx.last_screened() != 0                                          # the screening path really answered
    idx.close()


@pytest.mark.parametrize("metric", ["ip", "l2"])
def test_both_storage_paths_agree(rmu, corpus, metric):
    x, xl2, q = corpus
    xs = (xl2 if metric == "l2" else x)[:20_000]
    dead = _dead_rows(len(xs), np.random.default_rng(11), frac=0.4)
    out = {}
    for inplace in (False, True):
        idx = rmu.FlatIndex(384, metric=_metric(metric))
        idx.add(xs)
        idx.set_compact_inplace(inplace)
        idx.set_screen_min_batch(1)
        idx.remove_rows(dead)
        cap0 = idx.stats()["capacity"]
        assert idx.compaction_stats()["compact_count"] == 0
        m = idx.compact()
        st, cs = idx.stats(), idx.compaction_stats()
        assert cs["compact_count"] == 1 and cs["compact_ms"] > 0
        assert (st["capacity"] == cap0) if inplace else (st["capacity"] < cap0)
        out[inplace] = (m, idx.get_rows(np.arange(len(idx))), idx.search(q, 10), idx.search(q, 60))
        idx.close()
    a, b = out[False], out[True]
    assert np.array_equal(a[0], b[0])
    assert np.array_equal(a[1], b[1])
    live = np.setdiff1d(np.arange(len(xs)), dead)
    if metric == "ip":
        assert np.array_equal(a[1], xs[live])                                   # the stored rows themselves, in order
    for (s0, r0), (s1, r1) in zip(a[2:], b[2:]):
        assert np.array_equal(r0, r1) and np.array_equal(s0, s1)


@pytest.mark.parametrize("metric", ["ip", "l2"])
@pytest.mark.parametrize("n_live", [1, 31, 33, 159, 161])
def test_vacated_tail_reads_like_a_fresh_index(rmu, metric, n_live):
    """In place, a full 4096-row index whose LAST rows stay live: rows [n_live, 4096) held live data before and must read as a fresh
    index's zero rows now (the screening scan looks up to 159 rows past the last row)."""
    rng = np.random.default_rng(n_live)
    x = O.make_corpus(4096, seed=n_live)
    if metric == "l2":
        x = (x * rng.uniform(0.3, 3.0, (4096, 1))).astype(np.float32)
    q, _ = O.make_queries(x, 40, seed=5)
    live = np.sort(np.concatenate([np.arange(4096 - (n_live + 1) // 2, 4096),
                                   rng.choice(4096 - (n_live + 1) // 2, n_live - (n_live + 1) // 2, replace=False)]))
    assert live.size == n_live
    idx = rmu.FlatIndex(384, metric=_metric(metric), capacity_hint=4096)
    idx.add(x)
    idx.set_compact_inplace(True)
    idx.remove_rows(np.setdiff1d(np.arange(4096), live))
    idx.compact()
    assert idx.stats()["capacity"] == 4096 and len(idx) == n_live
    for path in ("screen", "exact"):
        _set_path(idx, path)
        k = min(10, n_live + 3)
        s, r = idx.search(q, k)
        _oracle_parity(s, r, q, x[live], k, _metric(metric))
    idx.close()


def test_edges(rmu, corpus, tmp_path):
    from ragmeup_amd import _native as N
    x, xl2, q = corpus
    lib = N.lib()
    # no dead row: identity map, nothing re-allocated, not counted
    idx = rmu.FlatIndex(384)
    idx.add(x[:5000])
    cap0 = idx.stats()["capacity"]
    assert np.array_equal(idx.compact(), np.arange(5000))
    assert idx.stats()["capacity"] == cap0 and idx.compaction_stats()["compact_count"] == 0
    # map_len too short: RMU_E_INVALID, nothing changes
    idx.remove_rows([3, 4000])
    s0, r0 = idx.search(q, 10)
    m = np.full(4999, 7, np.int64)
    after = ctypes.c_int64(-5)
    assert lib.rmu_index_compact(idx._h, m.ctypes.data, 4999, ctypes.byref(after)) == -1
    assert (m == 7).all() and after.value == -5 and len(idx) == 5000
    s1, r1 = idx.search(q, 10)
    assert np.array_equal(s0, s1) and np.array_equal(r0, r1)
    # a longer map: entries past the row count are -1; a null map is allowed
    m = np.full(5003, 7, np.int64)
    assert lib.rmu_index_compact(idx._h, m.ctypes.data, 5003, ctypes.byref(after)) == 0
    assert after.value == 4998 and (m[[3, 4000, 5000, 5001, 5002]] == -1).all() and m[4999] == 4997
    idx.remove_rows([0])
    assert lib.rmu_index_compact(idx._h, None, 0, ctypes.byref(after)) == 0 and after.value == 4997
    # add after compact continues at row n_live
    assert idx.add(x[5000:5010]) == 4997 and len(idx) == 5007
    live = np.concatenate([np.setdiff1d(np.arange(5000), [0, 3, 4000]), np.arange(5000, 5010)])
    s, r = idx.search(q, 10)
    _oracle_parity(s, r, q, x[live], 10, N.METRIC_IP)
    # save / load after compaction: the same rows and results
    p = str(tmp_path / "c.rmu")
    idx.save(p)
    back = rmu.FlatIndex.load(p)
    assert len(back) == 5007 and os.path.getsize(p) == 64 + 5007 + 5007 * 384 * 4
    assert np.array_equal(back.get_rows(np.arange(5007)), idx.get_rows(np.arange(5007)))
    s2, r2 = back.search(q, 10)
    assert np.array_equal(s2, s) and np.array_equal(r2, r)
    back.close(); idx.close()
    # every row dead, and the empty index
    for metric in ("ip", "l2"):
        for inplace in (False, True):
            idx = rmu.FlatIndex(384, metric=_metric(metric))
            idx.add(x[:3000])
            idx.set_compact_inplace(inplace)
            idx.remove_rows(np.arange(3000))
            m = idx.compact()
            assert (m == -1).all() and len(idx) == 0 and idx.stats()["live_rows"] == 0
            s, r = idx.search(q[:4], 10)
            assert (r == -1).all() and (np.isposinf(s) if metric == "l2" else np.isneginf(s)).all()
            assert idx.add(x[:5]) == 0
            s, r = idx.search(q[:4], 3)
            _oracle_parity(s, r, q[:4], x[:5], 3, _metric(metric))
            idx.close()
    empty = rmu.FlatIndex(384)
    assert empty.compact().shape == (0,) and len(empty) == 0
    empty.close()


def test_mmr_after_compaction(rmu, corpus):
    x, _, q = corpus
    idx = rmu.FlatIndex(384)
    idx.add(x[:30_000])
    dead = _dead_rows(30_000, np.random.default_rng(21))
    idx.remove_rows(dead)
    s, r = idx.search(q, 20)
    pos0 = idx.mmr(q, r, 8, 0.4)
    rows0, sc0 = idx.search_mmr(q, 20, 8, 0.4, row_base=0)
    m = idx.compact()
    s1, r1 = idx.search(q, 20)
    assert np.array_equal(r1, _mapped(r, m)) and np.array_equal(s1, s)
    assert np.array_equal(idx.mmr(q, r1, 8, 0.4), pos0)
    rows1, sc1 = idx.search_mmr(q, 20, 8, 0.4, row_base=0)
    assert np.array_equal(rows1, _mapped(rows0, m)) and np.array_equal(sc1, sc0)
    idx.close()


def test_fused_encoder_search_after_compaction(rmu, tmp_path):
    """rmu_bert_search_mmr through the store (retriever.invoke, similarity_search_with_score) after a delete / re-upload and compact():
    the same documents and scores as before the compaction."""
    from ragmeup_amd.bert import BertEncoder
    from ragmeup_amd.documents import Document
    from ragmeup_amd.embeddings import MI355XEmbeddings
    from ragmeup_amd.tokenizer import WordPieceTokenizer
    from ragmeup_amd.vectorstore import MI355XVectorStore
    from tests.helpers import bert_weights_numpy, make_bert, synth_texts, synth_vocab
    enc = BertEncoder(bert_weights_numpy(make_bert(seed=0, layers=6)), layers=6)
    vp = tmp_path / "vocab.txt"
    vp.write_text("\n".join(synth_vocab()) + "\n", encoding="utf-8")
    emb = MI355XEmbeddings(encoder=enc, tokenizer=WordPieceTokenizer(str(vp)), max_seq_length=128)
    texts = synth_texts(600, seed=5, wmin=10, wmax=40)
    store = MI355XVectorStore(embeddings=emb, collection_name="fused_compact", auto_persist=False)
    store.add_documents([Document(t, {"source": f"s{i % 3}"}) for i, t in enumerate(texts)], ids=[str(i) for i in range(600)])
    store.delete(expr='source == "s1"')
    store.add_documents([Document(t + " again", {"source": "s2"}) for t in texts[:100]], ids=[str(i) for i in range(100)])
    calls = []
    real = enc.search_host
    enc.search_host = lambda *a, **k: calls.append(1) or real(*a, **k)
    queries = synth_texts(6, seed=6, wmin=5, wmax=14)
    retr = store.as_retriever(search_type="mmr", search_kwargs={"k": 8})

    def results():
        return [([(d.metadata["pk"], d.page_content) for d in retr.invoke(qq)],
                 [(d.metadata["pk"], d.page_content, s) for d, s in store.similarity_search_with_score(qq, k=6)]) for qq in queries]
    try:
        before = results()
        n_before = len(store._index)
        assert store.compact() == n_before - len(store)
        assert len(store._index) == len(store)
        assert results() == before
        assert len(calls) == 2 * 2 * len(queries)                                # every query took the fused call
    finally:
        enc.search_host = real
        store._index.close()


def test_scale_2m_rows_both_paths(rmu):
    import torch
    n = 2_000_000
    g = torch.Generator(device="cuda").manual_seed(5)
    xd = torch.randn((n, 384), device="cuda", generator=g)
    xd /= xd.norm(dim=1, keepdim=True)
    pick = torch.randint(0, n, (1024,), device="cuda", generator=g)
    qd = xd[pick] + 0.1 * torch.randn((1024, 384), device="cuda", generator=g)
    qd /= qd.norm(dim=1, keepdim=True)
    q = qd.cpu().numpy()
    dead = np.sort(np.random.default_rng(9).choice(n, n // 10, replace=False))
    for inplace in (False, True):
        idx = rmu.FlatIndex(384)                          # grown to 2.69M rows: a compacted capacity of 2.03M is smaller
        idx.add(xd)
        idx.set_compact_inplace(inplace)
        idx.remove_rows(dead)
        s0, r0 = idx.search(q, 10)
        assert idx.last_screened() != 0
        cap0 = idx.stats()["capacity"]
        m = idx.compact()
        assert len(idx) == n - dead.size
        assert (idx.stats()["capacity"] == cap0) if inplace else (idx.stats()["capacity"] < cap0)
        s1, r1 = idx.search(q, 10)
        assert idx.last_screened() != 0
        assert np.array_equal(r1, _mapped(r0, m)) and np.array_equal(s1, s0)
        idx.close()
    del xd
    torch.cuda.empty_cache()


class HashEmbeddings:
    """Deterministic unit-norm embeddings of a text (no encoder): a returned score can be recomputed from the Document's own text."""

    def embed_documents(self, texts):
        return [self.vec(t).tolist() for t in texts]

    def embed_query(self, t):
        return self.vec(t).tolist()

    @staticmethod
    def vec(t):
        v = np.random.default_rng(int(hashlib.md5(t.encode()).hexdigest()[:8], 16)).standard_normal(384)
        return (v / np.linalg.norm(v)).astype(np.float32)


def _docs(n, version):
    from ragmeup_amd.documents import Document
    return [Document(f"doc {i} version {version}", {"source": f"f{i % 7}.pdf"}) for i in range(n)]


def test_store_reupload_loop_stays_bounded_and_equals_a_fresh_store(rmu):
    from ragmeup_amd.vectorstore import MI355XVectorStore
    n = 2000
    ids = [f"id{i}" for i in range(n)]
    st = MI355XVectorStore(embeddings=HashEmbeddings(), collection_name="reup", auto_persist=False, compact_threshold=0.5)
    for rnd in range(30):
        st.add_documents(_docs(n, rnd), ids=ids)
        assert len(st._index) <= 3 * n and st._index.stats()["capacity"] <= 8192
    assert len(st) == n and st._index.compaction_stats()["compact_count"] >= 14
    fresh = MI355XVectorStore(embeddings=HashEmbeddings(), collection_name="fresh", auto_persist=False)
    fresh.add_documents(_docs(n, 29), ids=ids)
    queries = [f"doc {i} version 29" for i in range(0, n, 97)] + ["unrelated query"]
    for qq in queries:
        a = [(d.metadata["pk"], d.page_content, s) for d, s in st.similarity_search_with_score(qq, k=10)]
        b = [(d.metadata["pk"], d.page_content, s) for d, s in fresh.similarity_search_with_score(qq, k=10)]
        assert a == b
        assert ([d.metadata["pk"] for d in st.max_marginal_relevance_search(qq, k=5)] ==
                [d.metadata["pk"] for d in fresh.max_marginal_relevance_search(qq, k=5)])
    st._index.close(); fresh._index.close()


def test_readers_during_compaction_never_get_the_wrong_document(rmu):
    """Four threads search while a writer deletes, re-uploads and compacts: every (Document, score) returned must belong together (the
    score recomputed from the Document's own text), and nothing raises."""
    from ragmeup_amd.vectorstore import MI355XVectorStore
    n = 3000
    ids = [f"id{i}" for i in range(n)]
    st = MI355XVectorStore(embeddings=HashEmbeddings(), collection_name="race", auto_persist=False)
    st.add_documents(_docs(n, 0), ids=ids)
    stop = threading.Event()
    errs, checked = [], [0]

    def reader(t):
        rng = np.random.default_rng(t)
        try:
            while not stop.is_set():
                qq = f"doc {int(rng.integers(n))} version {int(rng.integers(4))}"
                qv = HashEmbeddings.vec(qq).astype(np.float64)
                for d, s in st.similarity_search_with_score(qq, k=8):
                    ip = float(qv @ HashEmbeddings.vec(d.page_content).astype(np.float64))
                    assert abs(s - (2.0 - 2.0 * ip)) <= 1e-5, (qq, d.page_content, s, ip)
                    assert d.page_content.startswith(f"doc {d.metadata['pk'][2:]} ")
                    checked[0] += 1
                for d in st.max_marginal_relevance_search(qq, k=4, fetch_k=16):
                    assert d.page_content.startswith(f"doc {d.metadata['pk'][2:]} ")
        except Exception as e:   # noqa: BLE001
            errs.append(("reader", t, repr(e)))

    def writer():
        rng = np.random.default_rng(99)
        try:
            t_end, v = time.monotonic() + 2.0, 1
            while time.monotonic() < t_end:
                sel = np.sort(rng.choice(n, 300, replace=False))
                st.delete(ids=[ids[i] for i in sel[:150]])
                docs = _docs(n, v)
                st.add_documents([docs[i] for i in sel], ids=[ids[i] for i in sel])
                st.compact()
                v += 1
        except Exception as e:   # noqa: BLE001
            errs.append(("writer", repr(e)))
        finally:
            stop.set()

    ts = [threading.Thread(target=reader, args=(t,)) for t in range(4)] + [threading.Thread(target=writer)]
    [t.start() for t in ts]
    [t.join(timeout=120) for t in ts]
    assert not any(t.is_alive() for t in ts)
    assert not errs, errs[:5]
    assert checked[0] > 100 and st._index.compaction_stats()["compact_count"] >= 2
    assert len(st._index) == len(st) == n
    st._index.close()


def test_a_torch_graph_capture_on_another_thread_survives_compaction(rmu):
    """As the growth / removal test of test_search_gpu.py: while thread A is inside a torch.cuda.graph capture (global mode), thread B
    compacts an index -- out of place (hipMalloc / hipFree) and in place (staging buffer) -- and searches it; every capture replays with
    the right numbers and every search is exact."""
    import torch
    x = O.make_corpus(24_000)
    q, _ = O.make_queries(x, 32)
    a = torch.randn((256, 256), device="cuda")
    b = torch.randn((256, 256), device="cuda")
    ref = (a * b + 1.0).relu().cpu()
    torch.cuda.synchronize()
    dead = _dead_rows(24_000, np.random.default_rng(1))
    live = np.setdiff1d(np.arange(24_000), dead)
    want = O.flat_search(q, x[live], 12)
    errs = []
    for rnd, inplace in enumerate((False, True, False, True)):
        inside, proceed = threading.Event(), threading.Event()

        def capturer():
            try:
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    y = a * b
                    inside.set()
                    assert proceed.wait(120)
                    y = (y + 1.0).relu()
                g.replay()
                torch.cuda.synchronize()
                if not torch.allclose(y.cpu(), ref, atol=1e-3):
                    errs.append(("capture replay wrong", rnd))
            except Exception as e:   # noqa: BLE001
                errs.append(("capturer", rnd, repr(e)))
            finally:
                inside.set()

        def library_user():
            try:
                assert inside.wait(120)
                idx = rmu.FlatIndex(384)
                idx.add(x)
                idx.set_compact_inplace(inplace)
                idx.set_screen_min_batch(1)
                idx.remove_rows(dead)
                m = idx.compact()
                assert (m[live] == np.arange(live.size)).all()
                s, r = idx.search(q, 10)
                assert_topk_parity(s, r, *want)
                with tempfile.TemporaryDirectory() as tmp:
                    p = os.path.join(tmp, "c.rmu")
                    idx.save(p)
                    idx.close()
                    back = rmu.FlatIndex.load(p)
                    s2, r2 = back.search(q, 10)
                    assert np.array_equal(s2, s) and np.array_equal(r2, r)
                    back.close()
            except Exception as e:   # noqa: BLE001
                errs.append(("library", rnd, repr(e)))
            finally:
                proceed.set()

        ts = [threading.Thread(target=capturer), threading.Thread(target=library_user)]
        [t.start() for t in ts]
        [t.join() for t in ts]
        assert not errs, errs
