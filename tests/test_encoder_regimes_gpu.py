"""Every dispatch regime of the encoder forward (`enqueue_forward`, ragmeup_amd/csrc/bert.hip) against the fp64 oracle, on both
sides of each threshold.  The shapes and the regime each one selects are listed in tests/encoder_regimes.py, whose CPU guard
(tests/test_encoder_regimes_cpu.py) ties them to the thresholds in the source.

Bars (as tests/test_encoder_gpu.py): every compared token |h - h_ref| / |h_ref| <= 2e-2, and over >= 256 compared tokens the
mean of the signed error vectors (h - h_ref) / |h_ref| within 1.4e-3 (a systematic error the per-token bar cannot see); a pooled MEAN vector cosine >= 0.999
and, over >= 5 sequences, centred cosine >= 0.99; CLS vectors and un-normalised vectors held to the token bar (so their norm
within 2e-2); cross-encoder logits within 8e-3 (1 + |logit|).  Big batches are sampled for the oracle: the first, last, longest
and shortest sequences and those whose packed token range straddles a 16-token and a 128-token tile boundary always, a few
seeded others besides.  The oracle runs one sequence at a time at its own length (exactly what the masked batch computes).
"""
import zlib

import numpy as np
import pytest

from oracle import oracle as O
from tests import encoder_regimes as R
from tests.helpers import bert_weights_numpy, centred_cosine, make_bert

pytestmark = pytest.mark.gpu

H = R.HIDDEN
TOK_BAR = 2e-2
# The bf16 rounding noise of one token is ~0.8e-2 of its norm but points anywhere: averaged over a few hundred tokens it shrinks
# to a few 1e-4.  What stays is systematic -- the Linear weights rounded to bf16 once: 0.8-0.9e-3 measured over 700-1200 tokens
# of the 6-layer model -- or a kernel that computes the wrong thing by a little: a 1 % error in the out-proj / FFN2 bias of
# k_gemm_small or in k_ffn3's GELU output moves the mean error vector to 1.9-2.5e-3 while every token stays under 1.2e-2.
DRIFT_BAR = 1.4e-3
DRIFT_MIN_TOKENS = 256


class Model:
    """A BertEncoder, its weights, and a cache of oracle hidden states per (input key, sequence)."""

    def __init__(self, w, layers, eps=1e-12):
        from ragmeup_amd.bert import BertEncoder
        self.w, self.layers, self.eps = w, layers, eps
        self.enc = BertEncoder(w, layers=layers, ln_eps=eps)
        self._ref = {}

    def ref(self, key, ids, tt, lens, b):
        """oracle final hidden states [lens[b], H] of sequence b (lens already clipped, > 0)"""
        k = (key, b)
        if k not in self._ref:
            l = int(lens[b])
            t = np.zeros((1, l), np.int64) if tt is None else tt[b:b + 1, :l]
            self._ref[k] = O.bert_hidden(self.w, ids[b:b + 1, :l], t, np.array([l]), n_layers=self.layers, eps=self.eps)[0]
        return self._ref[k]


_MODELS = {}


def model(layers=6, head=False, short_pos=False):
    key = (layers, head, short_pos)
    if key not in _MODELS:
        import torch
        assert torch.cuda.is_available()
        w = bert_weights_numpy(make_bert(seed=1 if head else 0, layers=layers, head=head))
        if short_pos:       # a 128-row position table and layer_norm_eps = 1e-5 (an all-MiniLM-style config differs in both)
            w["embeddings.position_embeddings.weight"] = np.ascontiguousarray(w["embeddings.position_embeddings.weight"][:128])
            _MODELS[key] = Model(w, layers, eps=1e-5)
        else:
            _MODELS[key] = Model(w, layers)
    return _MODELS[key]


@pytest.fixture(scope="module", autouse=True)
def _free_models():
    yield
    for m in _MODELS.values():
        m.enc.close()
    _MODELS.clear()


# ---- inputs ------------------------------------------------------------------------------------------------------------------
def make_lens(case: R.Case, rng) -> np.ndarray:
    B, L = case.batch, case.max_len
    if case.lens == "full":
        return np.full(B, L, np.int32)
    if case.lens == "ramp":
        lens = rng.integers(1, L + 1, B).astype(np.int32)
        if B >= 2:
            lens[rng.permutation(B)[:2]] = (L, 1)
        else:
            lens[0] = L
        return lens
    assert case.lens == "groups"
    lens = np.zeros(B, np.int32)
    where = rng.permutation(B)
    i = 0
    for n, l in case.real:
        lens[where[i:i + n]] = l
        i += n
    return lens


def make_ids(lens, max_len, rng, pair=False):
    """[CLS] ... [SEP] rows; the padding holds random ids (a kernel that reads past a sequence would see them)"""
    B = len(lens)
    ids = rng.integers(1000, 30522, (B, max_len)).astype(np.int32)
    tt = np.zeros((B, max_len), np.int32) if pair else None
    for b, l in enumerate(np.minimum(lens, max_len)):
        if l > 1:                                  # (a one-token sequence keeps its random id: 2000 of them must differ)
            ids[b, 0] = 101
            ids[b, l - 1] = 102
            if pair and l >= 4:
                q = min(16, l // 2)
                ids[b, q] = 102
                tt[b, q + 1:l] = 1
    return ids, tt


def sample(lens, extra=4, seed=0):
    """Sequences to check against the oracle: all of a small batch; of a big one the first, last, longest, shortest (non-empty
    too), those straddling 16- and 128-token tile boundaries of the packed order (from cumsum(lens)), and `extra` seeded others."""
    lens = np.asarray(lens)
    B = len(lens)
    if B <= 12:
        return list(range(B))
    pick = {0, B - 1, int(np.argmax(lens)), int(np.argmin(lens))}
    nz = np.nonzero(lens > 0)[0]
    if nz.size:
        pick.add(int(nz[np.argmin(lens[nz])]))
    for tile in (16, 128):
        st = straddlers(lens, tile)
        if st:
            pick.update({st[0], st[len(st) // 2], st[-1]})
    rng = np.random.default_rng(seed)
    pool = nz if nz.size else np.arange(B)
    pick.update(int(b) for b in rng.choice(pool, min(extra, pool.size), replace=False))
    return sorted(pick)


def straddlers(lens, tile):
    """sequences whose packed token range [cu[b], cu[b+1]) has a multiple of `tile` strictly inside it"""
    cu = np.concatenate([[0], np.cumsum(lens)])
    return [b for b in range(len(lens)) if lens[b] > 1 and (cu[b + 1] - 1) // tile > cu[b] // tile]


def case_inputs(case: R.Case, pair=False):
    rng = np.random.default_rng(zlib.crc32(case.id.encode()))
    lens = make_lens(case, rng)
    ids, tt = make_ids(lens, case.max_len, rng, pair=pair)
    return ids, tt, lens


# ---- checks ------------------------------------------------------------------------------------------------------------------
def packed_rows(tok, lens, b):
    cu = np.concatenate([[0], np.cumsum(lens)])
    return tok[cu[b]:cu[b + 1]]


def check_tokens(m, key, ids, tt, lens, tok, sel, what):
    """Every token of the sampled sequences within TOK_BAR; over >= DRIFT_MIN_TOKENS of them, the mean relative error VECTOR
    within DRIFT_BAR (see there)."""
    assert tok.shape == (int(lens.sum()), H), (what, tok.shape)
    errs = []
    for b in sel:
        if lens[b] == 0:
            continue
        ref = m.ref(key, ids, tt, lens, b)
        got = packed_rows(tok, lens, b).astype(np.float64)
        e = (got - ref) / np.linalg.norm(ref, axis=1, keepdims=True)
        rel = np.linalg.norm(e, axis=1)
        assert rel.max() <= TOK_BAR, f"{what}: sequence {b} (len {lens[b]}): token {int(rel.argmax())} rel err {rel.max():.3e}"
        errs.append(e)
    if errs and sum(len(e) for e in errs) >= DRIFT_MIN_TOKENS:
        drift = float(np.linalg.norm(np.concatenate(errs).mean(0)))
        assert drift <= DRIFT_BAR, f"{what}: systematic error {drift:.3e} over {sum(len(e) for e in errs)} tokens"


def ref_pool(m, key, ids, tt, lens, b, cls, normalize):
    h = m.ref(key, ids, tt, lens, b)
    v = h[0] if cls else h.mean(0)
    return v / max(np.linalg.norm(v), 1e-12) if normalize else v


def check_pooled(m, key, ids, tt, lens, got, sel, mode, what):
    cls = (mode & 0xff) == R.MODE_CLS
    normalize = not (mode & R.NO_NORMALIZE)
    assert got.shape == (len(lens), H), (what, got.shape)
    assert np.isfinite(got).all(), what
    live = [b for b in sel if lens[b] > 0]
    for b in sel:
        if lens[b] == 0:
            assert not got[b].any(), f"{what}: empty sequence {b} pools to a non-zero vector"
    if not live:
        return
    g = got[live].astype(np.float64)
    r = np.stack([ref_pool(m, key, ids, tt, lens, b, cls, normalize) for b in live])
    cos = (g * r).sum(1) / np.linalg.norm(g, axis=1) / np.linalg.norm(r, axis=1)
    assert cos.min() >= 0.999, f"{what}: cosine {cos.min():.5f} at sequence {live[int(cos.argmin())]}"
    if normalize:
        assert np.allclose(np.linalg.norm(g, axis=1), 1.0, atol=1e-5), what
    if cls or not normalize:                       # one token's state / the raw mean: the token bar, which holds the norm too
        rel = np.linalg.norm(g - r, axis=1) / np.linalg.norm(r, axis=1)
        assert rel.max() <= TOK_BAR, f"{what}: rel err {rel.max():.3e} at sequence {live[int(rel.argmax())]}"
        ratio = np.linalg.norm(g, axis=1) / np.linalg.norm(r, axis=1)
        assert np.abs(ratio - 1).max() <= TOK_BAR, (what, ratio)
    if not cls and len(live) >= 5:                 # (every CLS state is the same token at the same position: nothing to centre)
        cc = centred_cosine(g, r)
        assert cc.min() >= 0.99, f"{what}: centred cosine {cc.min():.4f} at sequence {live[int(cc.argmin())]}"


def run(m, ids, lens, tt=None, mode=R.MODE_MEAN, out=None):
    return m.enc.encode_ids(ids, lens, tt, mode=mode, out=out).cpu().numpy()


POOL_MODES = [R.MODE_MEAN, R.MODE_MEAN | R.NO_NORMALIZE, R.MODE_CLS, R.MODE_CLS | R.NO_NORMALIZE]


# ---- every regime, from both sides of each threshold --------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.CASES, ids=[c.id for c in R.CASES])
def test_regime_vs_oracle(case):
    """MODE_TOKENS token by token and every pooling mode against the oracle; then the same sequences with one more padding column:
    bit-identical when that column leaves the regime unchanged, within the oracle bar on both sides when it crosses a threshold."""
    m = model(case.layers)
    ids, tt, lens = case_inputs(case)
    sel = sample(lens, seed=case.batch)
    tok = run(m, ids, lens, mode=R.MODE_TOKENS)
    check_tokens(m, case.id, ids, tt, lens, tok, sel, case.id)
    for mode in POOL_MODES:
        check_pooled(m, case.id, ids, tt, lens, run(m, ids, lens, mode=mode), sel, mode, f"{case.id} mode {mode:#x}")
    if case.max_len < m.enc.max_pos:
        rng = np.random.default_rng(case.batch)
        wide = np.concatenate([ids, rng.integers(1000, 30522, (case.batch, 1)).astype(np.int32)], axis=1)
        tok1 = run(m, wide, lens, mode=R.MODE_TOKENS)
        same = R.encoder_regime(case.batch, case.max_len, case.layers) == R.encoder_regime(case.batch, case.max_len + 1, case.layers)
        if same:
            assert np.array_equal(tok1, tok), f"{case.id}: one more padding column, same regime, different result"
        else:
            check_tokens(m, case.id, ids, tt, lens, tok1, sel, f"{case.id} + 1 padding column (crosses a threshold)")


def test_samples_include_the_tile_straddlers():
    """(the sampling rule above, on a ragged batch: what it must always pick)"""
    lens = np.array([5, 0, 20, 3, 120, 9, 0, 200, 1, 17, 16, 40, 7, 2], np.int32)
    sel = sample(lens)
    assert {0, len(lens) - 1, int(np.argmax(lens)), int(np.argmin(lens)), 8} <= set(sel)
    for tile in (16, 128):
        st = straddlers(lens, tile)
        assert st and st[0] in sel and st[-1] in sel, (tile, st, sel)


# ---- zero-length sequences --------------------------------------------------------------------------------------------------
ZERO_CASES = [("small", 8, 64, 6), ("tiled", 200, 256, 6), ("tiled-layers1", 200, 256, 1)]


@pytest.mark.parametrize("name,B,L,layers", ZERO_CASES, ids=[z[0] for z in ZERO_CASES])
def test_zero_length_sequences(name, B, L, layers):
    """Empty sequences first, in the middle and last: no token rows, a zero pooled vector (sentence-transformers' clamped mean),
    a finite logit; every other sequence as in the same batch without the empty ones (bit for bit: same regime)."""
    rng = np.random.default_rng(B * 7 + layers)
    lens = rng.integers(1, L + 1, B).astype(np.int32)
    lens[rng.integers(1, B - 1)] = L
    empty = [0, B // 2, B - 1]
    lens[empty] = 0
    ids, _ = make_ids(lens, L, rng)
    keep = np.array([b for b in range(B) if lens[b] > 0])
    assert R.encoder_regime(B, L, layers) == R.encoder_regime(len(keep), L, layers)
    m = model(layers)
    key = f"zero-{name}"
    ids_k, lens_k = np.ascontiguousarray(ids[keep]), np.ascontiguousarray(lens[keep])
    tok, tok_k = run(m, ids, lens, mode=R.MODE_TOKENS), run(m, ids_k, lens_k, mode=R.MODE_TOKENS)
    assert np.array_equal(tok, tok_k), name
    sel_k = sample(lens_k, seed=B)
    check_tokens(m, key, ids_k, None, lens_k, tok_k, sel_k, name)
    for mode in POOL_MODES:
        got, got_k = run(m, ids, lens, mode=mode), run(m, ids_k, lens_k, mode=mode)
        assert not got[empty].any(), (name, mode)
        assert np.array_equal(got[keep], got_k), (name, mode)
        check_pooled(m, key, ids_k, None, lens_k, got_k, sel_k, mode, f"{name} mode {mode:#x}")
    if layers == 6:
        c = model(6, head=True)
        ids_p, tt = make_ids(lens, L, rng, pair=True)
        lg, lg_k = run(c, ids_p, lens, tt, mode=R.MODE_CE), run(c, ids_p[keep], lens_k, tt[keep], mode=R.MODE_CE)
        assert np.isfinite(lg).all(), name
        assert np.array_equal(lg[keep], lg_k), name


# ---- lens > max_len ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,L", [(6, 100), (150, 256)], ids=["small-6x100", "tiled-150x256"])
def test_lens_past_max_len_are_clipped(B, L):
    rng = np.random.default_rng(B)
    lens = rng.integers(1, L + 1, B).astype(np.int32)
    lens[[0, B // 3, B - 1]] = (L + 1, L + 57, 1 << 20)
    ids, _ = make_ids(np.minimum(lens, L), L, rng)
    m = model(6)
    clipped = np.minimum(lens, L).astype(np.int32)
    for mode in (R.MODE_TOKENS, R.MODE_MEAN, R.MODE_CLS):
        assert np.array_equal(run(m, ids, lens, mode=mode), run(m, ids, clipped, mode=mode)), mode
    c = model(6, head=True)
    assert np.array_equal(run(c, ids, lens, mode=R.MODE_CE), run(c, ids, clipped, mode=R.MODE_CE))


# ---- caller output strides --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,L", [(9, 60), (140, 256)], ids=["small-9x60", "tiled-140x256"])
@pytest.mark.parametrize("width,col", [(385, 0), (512, 0), (512, 128), (512, 1)], ids=["w385", "w512", "w512-c128", "w512-c1"])
def test_pooled_into_a_slice_of_a_wider_matrix(B, L, width, col):
    """A row stride that is not a multiple of 4 (or a column offset that misaligns the rows) takes k_pool's scalar stores; the
    result equals the contiguous call and nothing outside the slice is written."""
    import torch
    rng = np.random.default_rng(B + width + col)
    lens = rng.integers(1, L + 1, B).astype(np.int32)
    ids, _ = make_ids(lens, L, rng)
    m = model(6)
    for mode in (R.MODE_MEAN, R.MODE_CLS | R.NO_NORMALIZE, R.MODE_TOKENS):
        ref = run(m, ids, lens, mode=mode)
        rows = ref.shape[0]
        big = torch.full((rows, width), -7.25, dtype=torch.float32, device=m.enc.device)
        m.enc.encode_ids(ids, lens, None, mode=mode, out=big[:, col:col + H])
        got = big.cpu().numpy()
        assert np.array_equal(got[:, col:col + H], ref), (mode, width, col)
        outside = np.concatenate([got[:, :col], got[:, col + H:]], axis=1)
        assert (outside == -7.25).all(), f"mode {mode:#x}: columns outside the slice were written"


# ---- pair inputs: token types on the tiled path ---------------------------------------------------------------------------
@pytest.mark.parametrize("B,L", [(14, 160), (140, 256)], ids=["small-14x160", "tiled-140x256"])
def test_pair_inputs_tokens_and_logits(B, L):
    c = model(6, head=True)
    rng = np.random.default_rng(B * 3)
    lens = rng.integers(8, L + 1, B).astype(np.int32)
    lens[rng.integers(B)] = L
    ids, tt = make_ids(lens, L, rng, pair=True)
    assert tt.any()
    key = f"pair-{B}x{L}"
    sel = sample(lens, extra=6, seed=B)
    tok = run(c, ids, lens, tt, mode=R.MODE_TOKENS)
    check_tokens(c, key, ids, tt, lens, tok, sel, key)
    lg = run(c, ids, lens, tt, mode=R.MODE_CE)
    ref = np.array([O.cross_encoder_logit(c.w, c.ref(key, ids, tt, lens, b)[None])[0] for b in sel])
    assert np.all(np.abs(lg[sel] - ref) <= 8e-3 * (1 + np.abs(ref))), (lg[sel], ref)
    # the token types matter: all-zero types give other states
    tok0 = run(c, ids, lens, np.zeros_like(tt), mode=R.MODE_TOKENS)
    assert not np.array_equal(tok0, tok)


# ---- layer_norm_eps = 1e-5 and a 128-row position table -----------------------------------------------------------------------
@pytest.mark.parametrize("B,L", [(10, 100), (300, 128)], ids=["small-10x100", "tiled-300x128"])
def test_short_position_table_and_ln_eps(B, L):
    from ragmeup_amd._native import RmuError
    m = model(6, short_pos=True)
    assert m.enc.max_pos == 128
    rng = np.random.default_rng(L)
    lens = rng.integers(1, L + 1, B).astype(np.int32)
    lens[rng.integers(B)] = L
    ids, _ = make_ids(lens, L, rng)
    key = f"eps-{B}x{L}"
    sel = sample(lens, seed=B)
    check_tokens(m, key, ids, None, lens, run(m, ids, lens, mode=R.MODE_TOKENS), sel, key)
    check_pooled(m, key, ids, None, lens, run(m, ids, lens, mode=R.MODE_MEAN), sel, R.MODE_MEAN, key)
    with pytest.raises(RmuError):                                    # max_len past the position table is refused
        run(m, np.zeros((1, 129), np.int32), np.array([129], np.int32), mode=R.MODE_MEAN)


# ---- the host entry point ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,L", R.HOST_CASES, ids=[f"host-{b}x{l}" for b, l in R.HOST_CASES])
def test_host_entry_point_at_each_bucket(B, L):
    """encode_host pads to a bucketed (bb, lb) -- on both sides of FOLD_TOKENS, up to HOST_TOKENS -- and replays a captured graph
    from its third call: every call equals encode_ids at the bucketed shape bit for bit, and the oracle within the bar."""
    rng = np.random.default_rng(B * 1000 + L)
    lens = rng.integers(1, L + 1, B).astype(np.int32)
    lens[0] = L
    ids, tt = make_ids(lens, L, rng, pair=True)
    m, c = model(6), model(6, head=True)
    bb, lb = m.enc.host_shape(B, L, R.MODE_MEAN)
    pi = np.zeros((bb, lb), np.int32)
    pi[:B, :L] = ids
    pt = np.zeros((bb, lb), np.int32)
    pt[:B, :L] = tt
    pl = np.zeros(bb, np.int32)
    pl[:B] = lens
    key = f"host-{B}x{L}"
    dev = run(m, pi, pl, mode=R.MODE_MEAN)[:B]
    for _ in range(3):                                               # eager, capture, replay
        assert np.array_equal(m.enc.encode_host(ids, lens, mode=R.MODE_MEAN), dev), (bb, lb)
    check_pooled(m, key, ids, None, lens, dev, list(range(B)), R.MODE_MEAN, key)
    dev_ce = run(c, pi, pl, pt, mode=R.MODE_CE)[:B]
    for _ in range(3):
        assert np.array_equal(c.enc.encode_host(ids, lens, tt, mode=R.MODE_CE), dev_ce), (bb, lb)
    sel = sample(lens, seed=B)
    ref = np.array([O.cross_encoder_logit(c.w, c.ref(key + "-ce", ids, tt, lens, b)[None])[0] for b in sel])
    assert np.all(np.abs(dev_ce[sel] - ref) <= 8e-3 * (1 + np.abs(ref))), (dev_ce[sel], ref)
    if m.enc.host_shape(B, L, R.MODE_TOKENS) is not None:
        tb, tl = m.enc.host_shape(B, L, R.MODE_TOKENS)
        tok = m.enc.encode_host(ids, lens, mode=R.MODE_TOKENS)
        ti = np.zeros((tb, tl), np.int32)
        ti[:B, :L] = ids
        assert np.array_equal(tok, run(m, ti, lens, mode=R.MODE_TOKENS))
        check_tokens(m, key, ids, None, lens, tok, list(range(B)), key + " tokens")
