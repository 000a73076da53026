"""GPU: the general encoder (csrc/bert_any.hip) -- BERTs with 64-wide heads, hidden 128..1024 -- against the fp64 oracle, token by token,
pooled, as cross-encoder logits and through the public surface.  The token bars are 2 x tests/anybert.MODEL_ERR (the error of the bf16
rounding model of those very kernels; the factor is the one the tuned path's bar, 2e-2, has to its model's 1.0e-2); the pooled and logit
bars are those of tests/test_encoder_gpu.py."""
import ctypes
import warnings

import numpy as np
import pytest

from ragmeup_amd.bert import MODE_CE, MODE_CLS, MODE_MEAN, MODE_TOKENS, NO_NORMALIZE
from tests import anybert as A
from tests.helpers import centred_cosine

pytestmark = pytest.mark.gpu

SETS = {"EDGE": lambda pair=False: A.edge_tokens(pair=pair), "9x40": lambda pair=False: A.synth_set(9, 40, pair=pair),
        "5x256": lambda pair=False: A.synth_set(5, 256, pair=pair), "3x512": lambda pair=False: A.synth_set(3, 512, pair=pair)}


@pytest.fixture(scope="module")
def models():
    """(name, layers, head) -> (BertEncoder, weights, geometry); one encoder per model for the module"""
    import torch
    assert torch.cuda.is_available()
    from ragmeup_amd.bert import BertEncoder
    cache = {}

    def get(name, layers=A.LAYERS, head=False, scale=None, seed=None):
        key = (name, layers, head, scale, seed)
        if key not in cache:
            if scale is None:
                geom, w = A.model_weights(name, layers, head=head)
            else:
                geom = A.GEOMS[name]
                w = A.make_weights(geom, layers, seed=seed, head=head, scale=scale)
            cache[key] = (BertEncoder(w, layers=layers, heads=geom[1], ffn=geom[2]), w, geom)
        return cache[key]
    yield get
    for enc, _, _ in cache.values():
        enc.close()


@pytest.fixture(scope="module")
def refs(models):
    """(name, layers, set) -> (tokens, packed oracle rows), computed once and never written to"""
    cache = {}

    def get(name, layers, set_name):
        key = (name, layers, set_name)
        if key not in cache:
            _, w, geom = models(name, layers)
            ids, tt, lens = SETS[set_name]()
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                ref = A.oracle_tokens(w, ids, tt, lens, geom, layers)
            ref.setflags(write=False)
            cache[key] = ((ids, tt, lens), ref)
        return cache[key]
    return get


CASES = [(n, A.LAYERS, s) for n in ("TINY", "ODD", "SMALL", "BASE", "LARGE", "TINY_SHARP") for s in ("EDGE", "9x40")] + \
        [("BASE", 12, "5x256"), ("LARGE", 4, "3x512")]


@pytest.mark.parametrize("name,layers,set_name", CASES, ids=[f"{n}-{l}-{s}" for n, l, s in CASES])
def test_token_states_vs_oracle(models, refs, name, layers, set_name):
    """every token's final hidden state: relative L2 error <= 2 x MODEL_ERR of its model.  TINY_SHARP: the weights on which a wrong softmax
    scale shows (test_anybert_cpu.py: test_the_bars_discriminate)."""
    enc, w, geom = models(name, layers)
    (ids, tt, lens), ref = refs(name, layers, set_name)
    got = enc.encode_ids(ids, lens, None, mode=MODE_TOKENS).cpu().numpy()
    assert got.shape == (int(lens.sum()), geom[0])
    assert np.isfinite(got).all()
    rel = A.rel_err(got, ref)
    bar = 2 * A.MODEL_ERR[name, layers]
    print(f"{name} x{layers} {set_name}: max rel {rel.max():.4e} mean {rel.mean():.4e} bar {bar:.4e}")
    assert rel.max() <= bar, (float(rel.max()), int(rel.argmax()), bar)
    assert not enc.fused and enc.HIDDEN == geom[0] and enc.host_shape(1, 16, MODE_MEAN) is None


@pytest.mark.parametrize("name", ["TINY", "BASE", "LARGE"])
@pytest.mark.parametrize("set_name", ["EDGE", "9x40"])
def test_pooled_embeddings_vs_oracle(models, refs, name, set_name):
    enc, w, geom = models(name)
    (ids, tt, lens), ref_t = refs(name, A.LAYERS, set_name)
    live = lens > 0
    for mode, cls in ((MODE_MEAN, False), (MODE_CLS, True)):
        for nn in (0, NO_NORMALIZE):
            got = enc.encode_ids(ids, lens, None, mode=mode | nn).cpu().numpy()
            ref = A.pooled_oracle(ref_t, lens, cls=cls, normalize=not nn)
            assert got.shape == (len(lens), geom[0])
            assert not got[~live].any()                                       # an empty sequence: the zero vector
            g, r = got[live].astype(np.float64), ref[live]
            cos = (g * r).sum(1) / np.linalg.norm(g, axis=1) / np.linalg.norm(r, axis=1)
            print(f"{name} {set_name} mode {mode | nn:#x}: min cos {cos.min():.6f} min centred {centred_cosine(g, r).min():.4f}")
            assert cos.min() >= 0.999, cos
            if not nn:
                assert np.allclose(np.linalg.norm(g, axis=1), 1.0, atol=1e-5)
            elif cls:       # un-normalised, the first token's state itself: its length is off by no more than that token's error bar
                assert np.abs(np.linalg.norm(g, axis=1) / np.linalg.norm(r, axis=1) - 1).max() <= 2 * A.MODEL_ERR[name, A.LAYERS]
            assert centred_cosine(g, r).min() >= 0.99                          # (both sets hold five sequences or more)


@pytest.mark.parametrize("name", ["TINY", "BASE"])
def test_cross_encoder_logits_vs_oracle(models, name):
    """one rerank call's worth of pairs (14, token types 0 / 1) at the standard weights: |d| <= 8e-3 (1 + |logit|)"""
    enc, w, geom = models(name, head=True)
    ids, tt, lens = A.synth_set(14, 160, seed=9, pair=True)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ref_t = A.oracle_tokens(w, ids, tt, lens, geom)
    ref = A.ce_oracle(w, ref_t, lens)
    got = enc.encode_ids(ids, lens, tt, mode=MODE_CE).cpu().numpy()
    print(f"{name}: max |d| / (1 + |ref|) {(np.abs(got - ref) / (1 + np.abs(ref))).max():.3e}; ref std {ref.std():.4f}")
    assert got.shape == (14,)
    assert np.all(np.abs(got - ref) <= 8e-3 * (1 + np.abs(ref))), (got, ref)
    rel = A.rel_err(enc.encode_ids(ids, lens, tt, mode=MODE_TOKENS).cpu().numpy(), ref_t)
    assert rel.max() <= 2 * A.MODEL_ERR[name, A.LAYERS], float(rel.max())      # token types 0 / 1 included
    # an empty pair: the head over a zero hidden state (include/rmu.h), the others unchanged bit for bit
    lens0 = lens.copy()
    lens0[3] = 0
    got0 = enc.encode_ids(ids, lens0, tt, mode=MODE_CE).cpu().numpy()
    zero = A.ce_oracle(w, np.zeros((1, geom[0])), np.array([1]))[0]
    assert abs(got0[3] - zero) <= 1e-5 and np.array_equal(np.delete(got0, 3), np.delete(got, 3))


@pytest.mark.parametrize("name", ["TINY", "BASE"])
def test_cross_encoder_logits_on_weights_that_do_not_collapse(models, name):
    """Linear weights x3 (tests/helpers.make_bert's reason: logits that spread): Pearson r >= 0.99 and |d| <= 3e-2 over the same 14 pairs"""
    enc, w, geom = models(name, head=True, scale=3.0, seed=1)
    ids, tt, lens = A.synth_set(14, 160, seed=9, pair=True)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        ref = A.ce_oracle(w, A.oracle_tokens(w, ids, tt, lens, geom), lens)
    got = enc.encode_ids(ids, lens, tt, mode=MODE_CE).cpu().numpy()
    print(f"{name} x3: max |d| {np.abs(got - ref).max():.3e}; ref std {ref.std():.4f}; r {np.corrcoef(got, ref)[0, 1]:.5f}")
    assert ref.std() > 0.08, float(ref.std())                                  # the weight set does what it is for
    assert np.corrcoef(got, ref)[0, 1] >= 0.99
    assert np.abs(got - ref).max() <= 3e-2, float(np.abs(got - ref).max())


def test_batch_and_padding_do_not_matter_bit_for_bit(models):
    for name in ("ODD", "BASE"):
        enc, _, _ = models(name)
        ids, tt, lens = A.edge_tokens()
        for mode in (MODE_TOKENS, MODE_MEAN):
            whole = enc.encode_ids(ids, lens, None, mode=mode).cpu().numpy()
            halves = np.concatenate([enc.encode_ids(ids[i:i + 6], lens[i:i + 6], None, mode=mode).cpu().numpy() for i in (0, 6)])
            assert np.array_equal(halves, whole)
            # one at a time (an empty sequence has no token rows to ask for: a call whose result is empty has no `out` to hand over)
            one = np.concatenate([enc.encode_ids(ids[i:i + 1, :max(int(lens[i]), 1)], lens[i:i + 1], None, mode=mode).cpu().numpy()
                                  for i in range(len(lens)) if mode != MODE_TOKENS or lens[i] > 0])
            assert np.array_equal(one, whole)
        assert ids.shape[1] == 512
        # garbage behind every sequence's end, and 37 more columns of it (max_len 475 + 37: lens are cut to the narrower call's width first)
        cut = np.minimum(lens, 475)
        a = enc.encode_ids(ids[:, :475], cut, None, mode=MODE_TOKENS).cpu().numpy()
        wide = np.concatenate([ids[:, :475], np.full((len(lens), 37), 999, np.int32)], axis=1)
        for b, l in enumerate(cut):
            wide[b, l:] = 999
        assert np.array_equal(enc.encode_ids(wide, cut, None, mode=MODE_TOKENS).cpu().numpy(), a)


def test_a_call_larger_than_the_token_group_equals_small_calls(models):
    """max_len 8: a group is GROUP_TOKENS / 8 = 2048 sequences; 2100 sequences cross into a second group once"""
    enc, _, geom = models("TINY")
    n = A.GROUP_TOKENS // 8 + 52
    ids, tt, lens = A.tokens_with_lens(np.random.default_rng(4).integers(0, 9, n), seed=6)
    assert ids.shape == (n, 8) and (lens == 0).any()
    for mode in (MODE_TOKENS, MODE_CLS):
        whole = enc.encode_ids(ids, lens, None, mode=mode).cpu().numpy()
        parts = np.concatenate([enc.encode_ids(ids[i:i + 525], lens[i:i + 525], None, mode=mode).cpu().numpy() for i in range(0, n, 525)])
        assert whole.shape == ((int(lens.sum()) if mode == MODE_TOKENS else n), geom[0])
        assert np.array_equal(whole, parts)


def test_two_forwards_queued_on_one_stream(models):
    import torch
    enc, _, geom = models("BASE")
    dev = enc.device
    sets = [A.synth_set(9, 40, seed=21), A.synth_set(5, 256, seed=22)]
    want = [enc.encode_ids(i, l, None, mode=MODE_MEAN).cpu().numpy() for i, _, l in sets]
    dids = [(torch.as_tensor(i, device=dev).contiguous(), torch.as_tensor(l, device=dev).contiguous()) for i, _, l in sets]
    outs = [torch.full((len(l), geom[0]), float("nan"), device=dev) for _, _, l in sets]
    torch.cuda.synchronize(dev)
    s = torch.cuda.Stream(dev)
    for (i, l), o in zip(dids, outs):
        enc.encode_ids(i, l, None, mode=MODE_MEAN, out=o, stream=s)          # left in flight, one behind the other
    after = enc.encode_ids(*sets[0][::2], None, mode=MODE_MEAN)              # stream 0: ordered behind both (tail event), complete on return
    s.synchronize()
    assert np.array_equal(outs[0].cpu().numpy(), want[0]) and np.array_equal(outs[1].cpu().numpy(), want[1])
    assert np.array_equal(after.cpu().numpy(), want[0])


def test_entry_points_of_the_tuned_geometry_refuse_a_general_model(models):
    from ragmeup_amd import FlatIndex, _native as N
    from ragmeup_amd.rerank import PassageTable
    enc, _, geom = models("TINY", head=True)
    lib = enc._lib
    idx = FlatIndex(geom[0], device=0)
    idx.add(np.eye(8, geom[0], dtype=np.float32))
    table = PassageTable(101, 102, 0, max_len=32)              # two passages of four tokens; the call below is valid but for the model
    ptok, poff = np.arange(1, 9, dtype=np.int32), np.array([0, 4, 8], np.int64)
    N.check(lib.rmu_passages_set(table._gen.h, 0, ptok.ctypes.data, poff.ctypes.data, 2), "rmu_passages_set")
    keys, q_tok, q_len = np.array([0, 1], np.int64), np.array([5, 6, 7], np.int32), np.array([3], np.int32)
    ids, tt, lens = A.synth_set(3, 16, seed=2)
    want = enc.encode_ids(ids, lens, None, mode=MODE_MEAN).cpu().numpy()
    out = np.zeros((3, geom[0]), np.float32)
    rows = np.zeros((3, 4), np.int64)
    groups = np.array([[0, -1, 1, 2]], np.int32)
    scores = np.zeros(2, np.float64)
    pos, rscore = np.zeros(2, np.int32), np.zeros(2, np.float32)
    p = lambda a: a.ctypes.data
    calls = {
        "rmu_bert_encode_host": lambda: lib.rmu_bert_encode_host(enc._h, p(ids), None, p(lens), 3, 16, MODE_MEAN, p(out), geom[0]),
        "rmu_bert_search_mmr": lambda: lib.rmu_bert_search_mmr(enc._h, idx._h, p(ids), None, p(lens), 3, 16, MODE_MEAN, 4, 4, 0.5, 0, p(rows), None, None),
        "rmu_bert_attribute": lambda: lib.rmu_bert_attribute(enc._h, p(ids), None, p(lens), 3, 16, MODE_MEAN, p(groups), 1, p(scores), None, None),
        "rmu_bert_rerank": lambda: lib.rmu_bert_rerank(enc._h, table._gen.h, p(q_tok), p(q_len), 1, 3, p(keys), 2, 2, 32, 2, p(pos), p(rscore), None),
    }
    for who, call in calls.items():
        assert call() == N.RMU_E_INVALID, who
        msg = lib.rmu_last_error().decode()
        assert who in msg and "rmu_bert_encode " in msg, msg
        assert np.array_equal(enc.encode_ids(ids, lens, None, mode=MODE_MEAN).cpu().numpy(), want)      # the model is none the worse
    assert enc.host_shape(3, 16, MODE_MEAN) is None and enc.host_shape(1, 16, MODE_CE) is None
    table.close()
    idx.close()
    with pytest.raises(ValueError, match="fused"):
        enc.search_host(None, ids, lens, MODE_MEAN, 4, 4)
    with pytest.raises(ValueError, match="fused"):
        enc.attribute_host(ids, lens, MODE_MEAN, groups)
    with pytest.raises(N.RmuError, match="out_stride < hidden"):
        import torch
        enc.encode_ids(torch.as_tensor(ids, device=enc.device), torch.as_tensor(lens, device=enc.device), None, mode=MODE_MEAN,
                       out=torch.empty((3, geom[0] - 8), device=enc.device), stream=torch.cuda.current_stream(enc.device))


# ---- through the public surface -----------------------------------------------------------------------------------------
def _hf_embed(w, geom, layers, vocab_file, texts, max_seq_length=512):
    import torch
    from tests.helpers import hf_tokenizer
    tok = hf_tokenizer(vocab_file, True)
    model = A.hf_model(w, geom, layers, False).float()
    out = np.empty((len(texts), geom[0]), np.float32)
    with torch.no_grad():
        for b0 in range(0, len(texts), 64):
            enc = tok([t.replace("\n", " ") for t in texts[b0:b0 + 64]], padding=True, truncation=True, max_length=max_seq_length, return_tensors="pt")
            h = model(input_ids=enc["input_ids"], attention_mask=enc["attention_mask"], token_type_ids=enc["token_type_ids"]).last_hidden_state
            mk = enc["attention_mask"].unsqueeze(-1).float()
            out[b0:b0 + 64] = torch.nn.functional.normalize((h * mk).sum(1) / mk.sum(1).clamp(min=1e-9), p=2, dim=1).numpy()
    return out


def test_embeddings_and_store_over_a_base_checkpoint_directory(tmp_path):
    import os
    from ragmeup_amd.embeddings import MI355XEmbeddings
    from ragmeup_amd.vectorstore import MI355XVectorStore
    from tests.helpers import synth_texts
    d = str(tmp_path / "base")
    w = A.write_dir(d, A.BASE, layers=2)
    emb = MI355XEmbeddings(model_dir=d)
    assert emb.encoder.hidden == 768 and not emb.encoder.fused and emb.pooling == "mean" and emb.normalize
    texts = synth_texts(40, seed=3)
    got = np.asarray(emb.embed_documents(texts), np.float32)
    ref = _hf_embed(w, A.BASE, 2, os.path.join(d, "vocab.txt"), texts)
    cos = (got * ref).sum(1) / np.linalg.norm(got, axis=1) / np.linalg.norm(ref, axis=1)
    print(f"embed_documents vs transformers: min cos {cos.min():.6f}")
    assert got.shape == (40, 768) and cos.min() >= 0.999
    q = np.asarray(emb.embed_query(texts[7]), np.float32)
    assert q.shape == (768,) and np.abs(q - got[7]).max() < 2e-3
    assert emb.query_ids(texts[7]) is None                                     # no one-call route for this geometry

    store = MI355XVectorStore(embeddings=emb, collection_name="anybert_base", auto_persist=False, device_fields=["src"])
    corpus = synth_texts(200, seed=5, wmin=10, wmax=40)
    store.add_texts(corpus, metadatas=[{"src": "a" if i % 2 else "b"} for i in range(200)], ids=[str(i) for i in range(200)])
    store.flush()
    try:
        assert store._index.dim == 768 and len(store._index) == 200
        for qt in synth_texts(3, seed=6, wmin=5, wmax=14):
            v = emb.embed_query_array(qt)
            g = store.similarity_search_with_score(qt, k=5)
            want = store.similarity_search_with_score_by_vector(v, 5)
            assert [(d_.page_content, s) for d_, s in g] == [(d_.page_content, s) for d_, s in want] and len(g) == 5
            _, rows = store._index.search(v[None], 5)
            assert [d_.page_content for d_, _ in g] == [corpus[r] for r in np.asarray(rows)[0]]
            m = [d_.page_content for d_ in store.max_marginal_relevance_search(qt, k=4, fetch_k=20)]
            assert m == [d_.page_content for d_ in store.max_marginal_relevance_search_by_vector(v, 4, 20, 0.5)] and len(m) == 4
            f = store.similarity_search_with_score(qt, k=5, expr='src == "a"')
            assert [(d_.page_content, s) for d_, s in f] == [(d_.page_content, s) for d_, s in
                                                             store.similarity_search_with_score_by_vector(v, 5, expr='src == "a"')]
            assert all(d_.metadata["src"] == "a" for d_, _ in f) and len(f) == 5
        qs = synth_texts(4, seed=8, wmin=5, wmax=14)
        retr = store.as_retriever(search_kwargs={"k": 3})
        assert [[d_.page_content for d_ in r] for r in retr.batch_invoke(qs)] == [[d_.page_content for d_ in retr.invoke(q_)] for q_ in qs]
    finally:
        store._index.close()
        emb.encoder.close()


def test_a_large_store_adds_and_searches(tmp_path):
    from ragmeup_amd.embeddings import MI355XEmbeddings
    from ragmeup_amd.vectorstore import MI355XVectorStore
    from tests.helpers import synth_texts
    d = str(tmp_path / "large")
    A.write_dir(d, A.LARGE, layers=1)
    emb = MI355XEmbeddings(model_dir=d)
    store = MI355XVectorStore(embeddings=emb, collection_name="anybert_large", auto_persist=False)
    corpus = synth_texts(64, seed=9)
    store.add_texts(corpus)
    store.flush()
    try:
        assert store._index.dim == 1024 and len(store._index) == 64
        hit = store.similarity_search(corpus[11], k=1)
        assert hit[0].page_content == corpus[11]
    finally:
        store._index.close()
        emb.encoder.close()


def test_cross_encoder_object_over_a_base_checkpoint_directory(tmp_path):
    import os
    import torch
    from ragmeup_amd.embeddings import MI355XCrossEncoder
    from tests.helpers import hf_tokenizer, synth_texts
    d = str(tmp_path / "base_ce")
    w = {k[5:] if k.startswith("bert.") else k: v for k, v in A.write_dir(d, A.BASE, layers=2, head=True).items()}
    ce = MI355XCrossEncoder(model_dir=d)
    assert ce.activation == "sigmoid" and not ce.encoder.fused
    query, passages = synth_texts(1, seed=1, wmin=4, wmax=9)[0], synth_texts(20, seed=2, wmin=10, wmax=50)
    pairs = [(query, t) for t in passages]
    got = np.asarray(ce.score(pairs))
    tok = hf_tokenizer(os.path.join(d, "vocab.txt"), True)
    enc = tok([p_[0] for p_ in pairs], [p_[1] for p_ in pairs], padding=True, truncation="longest_first", max_length=512, return_tensors="pt")
    with torch.no_grad():
        ref = torch.sigmoid(A.hf_model(w, A.BASE, 2, True)(**enc).logits[:, 0]).numpy()
    print(f"score vs transformers: max |d| {np.abs(got - ref).max():.3e}")
    assert np.abs(got - ref).max() <= 1e-2
    ce.activation = "identity"                                                # (rerank serves the identity activation)
    pos, sc = ce.rerank(query, passages, 5)
    assert ce._passages is None                                               # no passages table for this geometry
    logit = np.log(ref / (1 - ref))
    order = np.argsort(-logit, kind="stable")[:5]
    for a, b in zip(pos, order):
        assert a == b or abs(logit[a] - logit[b]) < 1e-2
    assert sc == sorted(sc, reverse=True) and len(pos) == 5
    ce.encoder.close()


def test_the_tuned_path_is_untouched_beside_a_general_model(models):
    from oracle import oracle as O
    from ragmeup_amd.bert import BertEncoder
    from tests.helpers import bert_weights_numpy, make_bert, synth_tokens, token_rel_error
    gen, _, _ = models("BASE")
    ids, tt, lens = A.synth_set(9, 40)
    gen.encode_ids(ids, lens, None, mode=MODE_MEAN)                           # a general model has run in this process
    w = bert_weights_numpy(make_bert(seed=0, layers=2))
    enc = BertEncoder(w, layers=2)
    try:
        assert enc.fused and enc.HIDDEN == 384 and enc.host_shape(1, 16, MODE_MEAN) == (1, 16)
        ids, tt, lens = synth_tokens(9, seed=22, lmin=2, lmax=40, mean=24, std=8)
        got = enc.encode_ids(ids, lens, None, mode=MODE_TOKENS).cpu().numpy()
        rel = token_rel_error(got, O.bert_hidden(w, ids, np.zeros_like(ids), lens, n_layers=2), lens)
        assert rel.max() <= 2e-2, float(rel.max())
        host = enc.encode_host(ids, lens, None, MODE_MEAN)
        assert host.shape == (9, 384) and np.abs(host - enc.encode_ids(ids, lens, None, mode=MODE_MEAN).cpu().numpy()).max() < 2e-3
    finally:
        enc.close()
