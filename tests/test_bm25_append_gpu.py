"""GPU: documents appended to a BM25 index whose image is in HBM (bm25.hip: bm25_splice_kernel; include/rmu.h, RMU_BM25_OPT_REPACK_ON_ADD).
Every case runs two handles through the same calls -- one that splices (the default) and one that repacks on every add (option 8 = 1, the path
before the splice existed) -- and asks that they agree bit for bit at k = 4 and k = 100 and that both properties of the live tests hold against
the fp64 formula over the live texts (tests/bm25_live.py).  Each case runs at the default geometry and at 64-document tiles on 3 workgroups."""
import numpy as np
import pytest

from tests.bm25_live import OPT_REPACK, OPT_TILE, OPT_WGS, LiveCorpus, check_all, same_bits
from tests.bm25_ref import synth_corpus, synth_queries
from tests.test_bm25_gpu import _query_set

pytestmark = pytest.mark.gpu

OPT_REPACK_ADD = 8
KS = (4, 100)
GEOMS = [(0, 0), (64, 3)]
_TEXTS: dict = {}
_REFS: dict = {}


def _texts(n=6572, seed=41):
    if (n, seed) not in _TEXTS:
        _TEXTS[n, seed] = synth_corpus(n, seed=seed)
    return _TEXTS[n, seed]


def _queries(texts):
    return _query_set(texts) + synth_queries(texts, 8, seed=12)


class Pair:
    """the splicing handle, the repacking handle and the live corpus, fed the same calls; `name` keys the fp64 references, which the two
    geometries of a case share"""

    def __init__(self, name, texts, tile, wgs, repack_on_remove=0):
        from ragmeup_amd.bm25 import BM25Index
        self.name, self.geom = name, (tile, wgs, repack_on_remove)
        self.ix, self.ref = BM25Index(), BM25Index()
        self.ref.set_option(OPT_REPACK_ADD, 1)
        for h in (self.ix, self.ref):
            self._options(h)
        self.c = LiveCorpus([])
        self.add(texts)

    def _options(self, h):
        h.set_option(OPT_TILE, self.geom[0])
        h.set_option(OPT_WGS, self.geom[1])
        h.set_option(OPT_REPACK, self.geom[2])

    def add(self, texts):
        first = len(self.c.texts)
        assert self.ix.add_texts(texts) == self.ref.add_texts(texts) == first
        self.c.add(texts)

    def remove(self, ids):
        assert self.ix.remove(ids) == self.ref.remove(ids) == self.c.remove(ids)

    def compact(self):
        want = self.c.compact()
        assert np.array_equal(self.ix.compact(), want) and np.array_equal(self.ref.compact(), want)

    def check(self, queries, **kw):
        key = (self.name, len(self.c.texts), self.c.alive.tobytes())
        if key in _REFS:
            self.c._ref = _REFS[key]
        _REFS[key] = self.c.ref
        assert self.ix.stat() == self.ref.stat()
        for k in KS:
            got = check_all(self.ix, self.c, queries, (k,), **kw)
            assert same_bits(got, self.ref.search(queries, k, **({"docs": kw["allow"]} if "allow" in kw else {}))), k

    def counts(self, h=None):
        st = (h or self.ix).image_stat()
        return st["packs"], st["splices"]

    def close(self):
        self.ix.close()
        self.ref.close()


@pytest.mark.parametrize("tile,wgs", GEOMS)
def test_a_chain_of_appends_takes_one_pack_and_five_splices(tile, wgs):
    texts = _texts()
    q = _queries(texts)
    p = Pair("chain", texts[:3000], tile, wgs)
    try:
        assert p.counts() == p.counts(p.ref) == (0, 0)
        p.check(q)
        at = 3000
        for n in (1, 7, 64, 500, 3000):
            p.add(texts[at:at + n])
            at += n
            p.check(q)
        assert at == len(texts)
        assert p.counts() == (1, 5) and p.counts(p.ref) == (6, 0)
    finally:
        p.close()


@pytest.mark.parametrize("tile,wgs", GEOMS)
def test_every_posting_list_equals_that_of_an_index_built_at_once(tile, wgs):
    from ragmeup_amd.bm25 import BM25Index
    base = _texts(500, seed=43)
    texts = base[:400] + [f"{t} fresh{i % 17} fresh{i % 17} only{i}" if i % 3 else f"only{i}" for i, t in enumerate(base[400:])]
    vocabulary = sorted(set(" ".join(texts).split()))
    assert len(set(" ".join(texts[400:]).split()) - set(" ".join(texts[:400]).split())) >= 100
    p = Pair("lists", texts[:400], tile, wgs)
    once = BM25Index()
    try:
        p._options(once)
        once.add_texts(texts)
        p.ix.search(vocabulary[:3], 4)
        p.ref.search(vocabulary[:3], 4)
        p.add(texts[400:])
        got = p.ix.search(vocabulary, 112)
        assert p.counts() == (1, 1)
        assert same_bits(got, once.search(vocabulary, 112)) and same_bits(got, p.ref.search(vocabulary, 112))
        check_all(p.ix, p.c, vocabulary[::7] + ["only5 fresh3 w0", "fresh16"], (112,))
    finally:
        once.close()
        p.close()


@pytest.mark.parametrize("tile,wgs", GEOMS)
def test_two_adds_between_searches_take_one_splice(tile, wgs):
    texts = _texts()
    q = _queries(texts)
    p = Pair("two_adds", texts[:1000], tile, wgs)
    try:
        p.check(q)
        p.add(texts[1000:1100])
        p.add(texts[1100:1133])
        p.check(q)
        assert p.counts() == (1, 1) and p.counts(p.ref) == (2, 0)
    finally:
        p.close()


def _removal(n):
    """a block across a tile boundary, a stride, the ends"""
    return np.unique(np.concatenate([np.arange(40, 200), np.arange(0, n, 7), [n - 1]]))


@pytest.mark.parametrize("tile,wgs", GEOMS)
@pytest.mark.parametrize("order", ["search_remove_add_search", "add_remove_added_search", "remove_search_add_search", "repack_on_remove"])
def test_removals_mixed_in(order, tile, wgs):
    texts = _texts()
    q = _queries(texts)
    p = Pair("mixed", texts[:2000], tile, wgs, repack_on_remove=int(order == "repack_on_remove"))
    try:
        p.check(q)
        if order == "search_remove_add_search":              # stale and grown: one splice, whose refresh serves both
            p.remove(_removal(2000))
            p.add(texts[2000:2300])
            want = (1, 1)
        elif order == "add_remove_added_search":              # the delta carries postings of documents that are already removed
            p.add(texts[2000:2300])
            p.remove(np.concatenate([np.arange(2000, 2300, 3), [2299, 5]]))
            want = (1, 1)
        elif order == "remove_search_add_search":
            p.remove(_removal(2000))
            p.check(q)
            assert p.counts() == (1, 0)
            p.add(texts[2000:2300])
            want = (1, 1)
        else:                                                 # the removal made the image dirty: the add leaves it so
            p.remove(_removal(2000))
            p.add(texts[2000:2300])
            want = (2, 0)
        p.check(q)
        assert p.counts() == want and p.counts(p.ref) == (2, 0)
        p.remove([0, 1, 2290])                                # and the spliced image goes on through the refresh path
        p.check(q)
        assert p.counts() == (want[0] + int(order == "repack_on_remove"), want[1])
    finally:
        p.close()


@pytest.mark.parametrize("tile,wgs", GEOMS)
def test_appends_without_postings_and_to_an_image_without_postings(tile, wgs):
    texts = _texts()
    q = _queries(texts)
    p = Pair("empty_delta", texts[:300], tile, wgs)
    try:
        p.check(q)
        nnz, up = p.ix.stat()["nnz"], p.ix.image_stat()["upload_bytes"]
        p.add(["", "   ", "\t\n", ""] * 3)                      # N grows, nnz does not
        p.check(q)
        assert p.ix.stat()["nnz"] == nnz and len(p.ix) == 312 and p.counts() == (1, 1)
        assert p.ix.image_stat()["upload_bytes"] - up == 16 * (p.ix.stat()["vocab"] + 1)
    finally:
        p.close()
    p = Pair("empty_image", ["", " "] * 35, tile, wgs)
    try:
        p.check(q)
        assert p.ix.stat()["nnz"] == 0 and p.counts() == (1, 0)
        p.add(["", ""])                                         # nothing on either side
        p.check(q)
        assert p.ix.stat()["nnz"] == 0 and p.counts() == (1, 1)
        p.add(texts[:200])
        p.check(q)
        assert p.counts() == (1, 2) and p.ix.stat()["nnz"] > 0
    finally:
        p.close()


@pytest.mark.parametrize("tile,wgs", GEOMS)
def test_after_a_compact_and_after_a_load_a_pack_then_splices_again(tile, wgs, tmp_path):
    from ragmeup_amd.bm25 import BM25Index
    texts = _texts()
    q = _queries(texts)
    p = Pair("compact_load", texts[:1500], tile, wgs)
    try:
        p.check(q)
        p.add(texts[1500:1600])
        p.check(q)
        assert p.counts() == (1, 1)
        p.remove(_removal(1600))
        p.compact()
        p.check(q)
        assert p.counts() == (2, 1)
        p.add(texts[1600:1700])
        p.check(q)
        assert p.counts() == (2, 2)
        path = str(tmp_path / "ix.bm25")
        p.ix.save(path)
        back = BM25Index.load(path)
        try:
            p._options(back)
            assert back.image_stat() == {"packs": 0, "splices": 0, "upload_bytes": 0}
            assert same_bits(back.search(q, 100), p.ref.search(q, 100)) and p.counts(back) == (1, 0)
            back.add_texts(texts[1700:1800])
            p.add(texts[1700:1800])
            p.check(q)
            assert same_bits(back.search(q, 100), p.ref.search(q, 100)) and p.counts(back) == (1, 1)
        finally:
            back.close()
    finally:
        p.close()


@pytest.mark.parametrize("tile,wgs", GEOMS)
def test_a_filtered_search_is_the_first_search_after_an_append(tile, wgs):
    texts = _texts()
    q = _queries(texts)
    p = Pair("subset", texts[:2000], tile, wgs)
    try:
        p.check(q)
        p.add(texts[2000:2500])
        allow = np.unique(np.concatenate([np.arange(3, 2500, 5), np.arange(1990, 2070)]))
        p.check(q, allow=allow)                                  # rmu_bm25_search_subset splices
        assert p.counts() == (1, 1)
        p.check(q)
        assert p.counts() == (1, 1)
    finally:
        p.close()


@pytest.mark.parametrize("tile,wgs", GEOMS)
def test_the_hybrid_call_is_the_first_search_after_an_append(tile, wgs):
    """tests/test_hybrid_gpu.py's check -- one call equals the member calls fused -- where the one call is what meets the grown image"""
    from ragmeup_amd import FlatIndex
    from ragmeup_amd.hybrid import HybridIndex, content_keys
    from tests.test_hybrid_gpu import _expected, _HashEmbeddings, _same
    texts = [t for t in _texts(700, seed=47) if t]
    first = 400
    emb = _HashEmbeddings()
    queries = synth_queries(texts, 16, seed=3)
    qv = np.asarray(emb.embed_documents(queries), np.float32)
    classes: dict = {}
    keys = content_keys(texts, classes)
    p = Pair("hybrid", texts[:first], tile, wgs)
    idx = FlatIndex(64)
    h = HybridIndex(p.ix, idx)
    try:
        idx.add(np.asarray(emb.embed_documents(texts[:first]), np.float32))
        h.set_keys(0, 0, keys[:first])
        h.set_keys(1, 0, keys[:first])
        h.search(qv, queries, 4, 20, 4)
        p.ref.search(queries, 4)
        assert p.counts() == (1, 0)
        p.add(texts[first:])
        idx.add(np.asarray(emb.embed_documents(texts[first:]), np.float32))
        h.set_keys(0, first, keys[first:])
        h.set_keys(1, first, keys[first:])
        for ks, fetch_k, kd in ((4, 20, 4), (100, 64, 64)):
            got = h.search(qv, queries, ks, fetch_k, kd, 0.5, (0.5, 0.5))
            assert p.counts() == (1, 1)
            docs = p.ref.search(queries, ks)[1]                  # the repacking handle's list ...
            assert np.array_equal(docs, p.ix.search(queries, ks)[1])
            rows = idx.search_mmr(qv, fetch_k, kd, 0.5)[0]
            _same(got, _expected(docs, rows, keys, keys, (0.5, 0.5)), (ks, fetch_k, kd))
        assert (docs >= first).any()
    finally:
        h.close()
        idx.close()
        p.close()


@pytest.mark.parametrize("tile,wgs", GEOMS)
def test_an_append_uploads_its_own_postings_and_two_pointer_arrays_at_most(tile, wgs):
    """the bound follows from the design: 8 bytes per added posting (document id, tf) and two u64 arrays of V_new + 1 pointers"""
    texts = _texts()
    q = _queries(texts)
    p = Pair("upload", texts[:3000], tile, wgs)
    try:
        p.ix.search(q, 4)
        p.ref.search(q, 4)
        st0, up0, ref0 = p.ix.stat(), p.ix.image_stat()["upload_bytes"], p.ref.image_stat()["upload_bytes"]
        assert up0 == ref0 == 8 * st0["nnz"]
        p.add(texts[3000:3050])
        p.check(q)
        st1 = p.ix.stat()
        d_nnz = st1["nnz"] - st0["nnz"]
        assert d_nnz > 0 and p.counts() == (1, 1)
        assert p.ix.image_stat()["upload_bytes"] - up0 <= 8 * d_nnz + 16 * (st1["vocab"] + 2)
        assert p.ref.image_stat()["upload_bytes"] - ref0 == 8 * st1["nnz"]
    finally:
        p.close()
