"""Helpers of the general-encoder tests (test_anybert_cpu.py, test_anybert_gpu.py): synthetic BERTs with 64-wide heads as plain numpy
dicts, the fp64 oracle over packed tokens, and `rounded_forward`, the error MODEL of csrc/bert_any.hip.  numpy only (no transformers model is built)."""
from __future__ import annotations

import numpy as np

TINY = (128, 2, 512)        # hidden, heads, ffn
ODD = (192, 3, 704)         # N = 192 / 576 / 704: none a multiple of the GEMM's 128-feature tile
SMALL = (512, 8, 2048)
BASE = (768, 12, 3072)
LARGE = (1024, 16, 4096)
GEOMS = {"TINY": TINY, "ODD": ODD, "SMALL": SMALL, "BASE": BASE, "LARGE": LARGE}
VOCAB = 1000
LAYERS = 2
GROUP_TOKENS = 16384        # csrc/bert_any.hip: a call is walked in groups of GROUP_TOKENS // max_len sequences

EDGE_LENS = [1, 2, 33, 63, 64, 65, 127, 129, 0, 511, 512, 7]      # 1614 tokens: no multiple of any tile, one empty sequence


def weight_names(layers, head=False):
    from ragmeup_amd.bert import weight_order
    return weight_order(layers, head)


def make_weights(geom, layers=LAYERS, seed=0, head=False, scale=1.0, vocab=VOCAB, max_pos=512):
    """HF parameter name -> fp32 array of a random BERT of this geometry: Linear weights N(0, 0.02 scale), embeddings N(0, 0.02), LayerNorm
    gains 1 + 0.05 N, LayerNorm and Linear biases 0.05 N (tests/helpers.make_bert's perturbation: a swapped gamma/beta or a dropped bias
    shows).  No transformers model is built."""
    hidden, heads, ffn = geom
    rng = np.random.default_rng(seed)
    n = lambda *s: rng.standard_normal(s).astype(np.float32)
    w = {"embeddings.word_embeddings.weight": 0.02 * n(vocab, hidden), "embeddings.position_embeddings.weight": 0.02 * n(max_pos, hidden),
         "embeddings.token_type_embeddings.weight": 0.02 * n(2, hidden),
         "embeddings.LayerNorm.weight": 1 + 0.05 * n(hidden), "embeddings.LayerNorm.bias": 0.05 * n(hidden)}
    lin = np.float32(0.02 * scale)
    for l in range(layers):
        p = f"encoder.layer.{l}."
        for name, (o, i) in (("attention.self.query", (hidden, hidden)), ("attention.self.key", (hidden, hidden)),
                             ("attention.self.value", (hidden, hidden)), ("attention.output.dense", (hidden, hidden)),
                             ("intermediate.dense", (ffn, hidden)), ("output.dense", (hidden, ffn))):
            w[p + name + ".weight"] = lin * n(o, i)
            w[p + name + ".bias"] = 0.05 * n(o)
        for name in ("attention.output.LayerNorm", "output.LayerNorm"):
            w[p + name + ".weight"] = 1 + 0.05 * n(hidden)
            w[p + name + ".bias"] = 0.05 * n(hidden)
    if head:
        w["pooler.dense.weight"] = lin * n(hidden, hidden)
        w["pooler.dense.bias"] = 0.05 * n(hidden)
        w["classifier.weight"] = lin * n(1, hidden)
        w["classifier.bias"] = 0.05 * n(1)
    return {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in w.items()}


def write_dir(d, geom, layers=2, head=False, st_files=True, binfile=False, pool_dim=None):
    """config.json + weights + tokenizer files (+ the sentence-transformers files) of a synthetic BERT of this geometry"""
    import json
    import os
    from tests.helpers import _write_tokenizer_files, synth_vocab
    os.makedirs(d, exist_ok=True)
    hidden, heads, ffn = geom
    w = make_weights(geom, layers, head=head, vocab=len(synth_vocab()))
    cfg = {"model_type": "bert", "architectures": ["BertForSequenceClassification" if head else "BertModel"], "hidden_size": hidden,
           "num_hidden_layers": layers, "num_attention_heads": heads, "intermediate_size": ffn, "hidden_act": "gelu",
           "max_position_embeddings": 512, "type_vocab_size": 2, "vocab_size": len(synth_vocab()), "layer_norm_eps": 1e-12,
           "position_embedding_type": "absolute"}
    if head:
        cfg["id2label"] = {"0": "LABEL_0"}
        cfg["sbert_ce_default_activation_function"] = "torch.nn.modules.activation.Sigmoid"
        w = {(k if k.startswith("classifier.") else "bert." + k): v for k, v in w.items()}
    json.dump(cfg, open(os.path.join(d, "config.json"), "w"))
    if binfile:
        import torch
        torch.save({k: torch.from_numpy(v) for k, v in w.items()}, os.path.join(d, "pytorch_model.bin"))
    else:
        from safetensors.numpy import save_file
        save_file(w, os.path.join(d, "model.safetensors"))
    _write_tokenizer_files(d)
    if st_files and not head:
        mods = [{"idx": 0, "name": "0", "path": "", "type": "sentence_transformers.models.Transformer"},
                {"idx": 1, "name": "1", "path": "1_Pooling", "type": "sentence_transformers.models.Pooling"},
                {"idx": 2, "name": "2", "path": "2_Normalize", "type": "sentence_transformers.models.Normalize"}]
        json.dump(mods, open(os.path.join(d, "modules.json"), "w"))
        json.dump({"max_seq_length": 512, "do_lower_case": False}, open(os.path.join(d, "sentence_bert_config.json"), "w"))
        os.makedirs(os.path.join(d, "1_Pooling"), exist_ok=True)
        json.dump({"word_embedding_dimension": pool_dim or hidden, "pooling_mode_cls_token": False, "pooling_mode_mean_tokens": True,
                   "pooling_mode_max_tokens": False, "pooling_mode_mean_sqrt_len_tokens": False}, open(os.path.join(d, "1_Pooling", "config.json"), "w"))
    return w


def hf_model(w, geom, layers, head):
    """transformers' BertModel / BertForSequenceClassification (eager attention, fp64, eval) holding the weights of a make_weights dict"""
    import torch
    from transformers import BertConfig, BertForSequenceClassification, BertModel
    hidden, heads, ffn = geom
    cfg = BertConfig(vocab_size=w["embeddings.word_embeddings.weight"].shape[0], hidden_size=hidden, num_hidden_layers=layers,
                     num_attention_heads=heads, intermediate_size=ffn, max_position_embeddings=512, type_vocab_size=2, layer_norm_eps=1e-12,
                     hidden_act="gelu", attn_implementation="eager")
    if head:
        cfg.num_labels = 1
        m = BertForSequenceClassification(cfg)
        state = {("classifier." + k[len("classifier."):] if k.startswith("classifier.") else "bert." + k): torch.from_numpy(v) for k, v in w.items()}
    else:
        m = BertModel(cfg, add_pooling_layer=False)
        state = {k: torch.from_numpy(v) for k, v in w.items()}
    missing, unexpected = m.load_state_dict(state, strict=False)
    assert not unexpected and all("position_ids" in k for k in missing), (missing, unexpected)
    return m.double().eval()


# ---- token sets ----------------------------------------------------------------------------------------------------------
def tokens_with_lens(lens, seed=11, vocab=VOCAB, pair=False):
    """ids / type ids [n, max(lens)] int32 (ids below `vocab`, zero behind a sequence's end), lens int32.  pair: types 0 / 1 split at a third."""
    lens = np.asarray(lens, dtype=np.int32)
    rng = np.random.default_rng(seed)
    L = max(1, int(lens.max()))
    ids = np.zeros((len(lens), L), np.int32)
    tt = np.zeros((len(lens), L), np.int32)
    for i, l in enumerate(lens):
        ids[i, :l] = rng.integers(1, vocab, l)
        if pair:
            tt[i, max(1, l // 3):l] = 1
    return ids, tt, lens


def edge_tokens(seed=11, pair=False):
    return tokens_with_lens(EDGE_LENS, seed=seed, pair=pair)


def synth_set(n, L, seed=5, pair=False):
    """n sequences of 1..L tokens, the first of them L long (the call's max_len is L)"""
    rng = np.random.default_rng(seed)
    lens = rng.integers(1, L + 1, n)
    lens[0] = L
    return tokens_with_lens(lens, seed=seed + 1, pair=pair)


def pack(ref, lens):
    return np.concatenate([np.asarray(ref[b, :l], np.float64) for b, l in enumerate(lens)]) if len(lens) else np.zeros((0, ref.shape[-1]))


def rel_err(got, ref):
    """per-token relative L2 error of packed rows"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return np.linalg.norm(got - ref, axis=1) / np.linalg.norm(ref, axis=1)


def oracle_tokens(w, ids, types, lens, geom, layers=LAYERS):
    """oracle.bert_hidden over the call, packed [sum(lens), hidden] fp64.  Every sequence goes through the oracle on its own, cut to its
    length: the oracle's sequences are independent, its key mask makes padding invisible, and an empty sequence (softmax over nothing) has no rows."""
    from oracle import oracle as O
    out = []
    for b, l in enumerate(np.asarray(lens)):
        if l > 0:
            out.append(O.bert_hidden(w, ids[b:b + 1, :l], types[b:b + 1, :l], np.array([l]), n_layers=layers, n_heads=geom[1])[0])
    return np.concatenate(out) if out else np.zeros((0, geom[0]))


# ---- the error model --------------------------------------------------------------------------------------------------
def bf16_round(x):
    """nearest-even rounding to bf16 (through fp32, as the kernels' fp32 accumulators are rounded), back as fp64"""
    a = np.ascontiguousarray(np.asarray(x, dtype=np.float32))
    u = a.view(np.uint32).astype(np.uint64)
    u = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    return u.astype(np.uint32).view(np.float32).reshape(a.shape).astype(np.float64)


def _ln(x, g, b, eps):
    mu = x.mean(-1, keepdims=True)
    var = ((x - mu) ** 2).mean(-1, keepdims=True)
    return (x - mu) / np.sqrt(var + eps) * g + b


MUTATIONS = ("drop_head", "swap_ln", "drop_bias", "mask_off_by_one", "scale32")


def rounded_forward(w, ids, types, lens, geom, layers=LAYERS, eps=1e-12, mutate=None, rounding=True):
    """oracle.bert_hidden in fp64 over packed tokens, with values rounded to bf16 exactly where csrc/bert_any.hip stores or converts bf16
    (-> packed [sum(lens), hidden] fp64).  The rounding points, each beside the kernel line that rounds there:
      weights            every Linear weight, Wq after the multiplication by log2(e) / 8 in fp32      k_any_to_bf16: `dst[i] = (bf16)(src[i] * scale)`
      h (embeddings)     LayerNorm(word + position + type), fp32 tables                                store_row_any: `o[i] = (bf16)v[u][i]` (k_any_embed_ln)
      qkv                h Wqkv^T + bias (bq scaled in fp32, not rounded)                              k_gemm_any epilogue: `o[r] = (bf16)v[r]` (EPI_BIAS)
      P                  2^(s - max) per key, in front of P V; the row sum l uses the UNROUNDED values   k_any_attn: `pb[j] = (bf16)sc[8 * s + j]`
      ctx                (P V) / l                                                                     k_any_attn: `a[e] = (bf16)(o0[4 * g + e] * inv)`
      y (twice a layer)  out-projection / FFN down + bias + residual, BEFORE its LayerNorm               k_gemm_any epilogue (EPI_RESID)
      h1, h              the two LayerNorms' outputs                                                   store_row_any (k_any_layernorm)
      mid                GELU(erf)(h1 W1^T + b1)                                                       k_gemm_any epilogue (EPI_GELU)
    Left out (what the factor 2 of the GPU bars is for): fp32 summation order, the device's exp2 / erf / rsqrt, and the online softmax's
    rounding of P against the RUNNING maximum of its 32-key tiles where this model rounds against the row's final maximum.
    mutate: one of MUTATIONS -- a deliberately wrong forward, for the tests that show the bars discriminate.  rounding=False: no rounding at all."""
    from scipy.special import erf
    hidden, heads, ffn = geom
    r = bf16_round if rounding else (lambda x: np.asarray(x, np.float64))
    f32 = lambda name: np.asarray(w[name], dtype=np.float32)
    f = lambda name: np.asarray(w[name], dtype=np.float64)
    lens = np.asarray(lens)
    cu = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    rows_b = np.repeat(np.arange(len(lens)), lens)
    rows_p = np.concatenate([np.arange(l) for l in lens]) if len(lens) else np.zeros(0, np.int64)
    tok, typ = ids[rows_b, rows_p], types[rows_b, rows_p]
    e = f("embeddings.word_embeddings.weight")[tok] + f("embeddings.position_embeddings.weight")[rows_p] + f("embeddings.token_type_embeddings.weight")[typ]
    h = r(_ln(e, f("embeddings.LayerNorm.weight"), f("embeddings.LayerNorm.bias"), eps))
    qs32 = np.float32(1.4426950408889634) / np.sqrt(np.float32(64.0))
    if mutate == "scale32":
        qs32 = np.float32(1.4426950408889634) / np.sqrt(np.float32(32.0))
    for l in range(layers):
        p = f"encoder.layer.{l}."
        first = l == 0
        wq = r(f32(p + "attention.self.query.weight") * qs32)
        bq = (f32(p + "attention.self.query.bias") * qs32).astype(np.float64)
        q = r(h @ wq.T + bq)
        k = r(h @ r(f(p + "attention.self.key.weight")).T + f(p + "attention.self.key.bias"))
        v = r(h @ r(f(p + "attention.self.value.weight")).T + f(p + "attention.self.value.bias"))
        ctx = np.zeros_like(h)
        for b, n in enumerate(lens):
            if n == 0:
                continue
            sl = slice(cu[b], cu[b] + n)
            qh = q[sl].reshape(n, heads, 64).transpose(1, 0, 2)
            kh = k[sl].reshape(n, heads, 64).transpose(1, 0, 2)
            vh = v[sl].reshape(n, heads, 64).transpose(1, 0, 2)
            s = qh @ kh.transpose(0, 2, 1)                       # log2 domain: the scale sits in Wq
            if mutate == "mask_off_by_one" and first and n > 1:
                s[:, :, n - 1] = -np.inf                         # the last real key is masked
            pr = np.exp2(s - s.max(-1, keepdims=True))
            c = (r(pr) @ vh) / pr.sum(-1, keepdims=True)
            if mutate == "drop_head" and first:
                c[0] = 0.0
            ctx[sl] = c.transpose(1, 0, 2).reshape(n, hidden)
        ctx = r(ctx)
        bo = f(p + "attention.output.dense.bias")
        if mutate == "drop_bias" and first:
            bo = np.zeros_like(bo)
        y = r(ctx @ r(f(p + "attention.output.dense.weight")).T + bo + h)
        g1, b1 = f(p + "attention.output.LayerNorm.weight"), f(p + "attention.output.LayerNorm.bias")
        if mutate == "swap_ln" and first:
            g1, b1 = b1, g1
        h1 = r(_ln(y, g1, b1, eps))
        x = h1 @ r(f(p + "intermediate.dense.weight")).T + f(p + "intermediate.dense.bias")
        mid = r(0.5 * x * (1.0 + erf(x / np.sqrt(2.0))))
        y = r(mid @ r(f(p + "output.dense.weight")).T + f(p + "output.dense.bias") + h1)
        h = r(_ln(y, f(p + "output.LayerNorm.weight"), f(p + "output.LayerNorm.bias"), eps))
    return h


def pooled_oracle(tokens, lens, cls=False, normalize=True):
    """sentence-transformers Pooling (masked mean | first token) + Normalize over packed oracle rows; an empty sequence gives the zero vector"""
    cu = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    out = np.zeros((len(lens), tokens.shape[1]))
    for b, n in enumerate(lens):
        if n > 0:
            out[b] = tokens[cu[b]] if cls else tokens[cu[b]:cu[b] + n].mean(0)
    if normalize:
        out = out / np.maximum(np.linalg.norm(out, axis=1, keepdims=True), 1e-12)
    return out


def ce_oracle(w, tokens, lens):
    """BertForSequenceClassification(num_labels = 1) over packed oracle rows (oracle.cross_encoder_logit on each sequence's first row)"""
    from oracle import oracle as O
    cu = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    cls = np.stack([tokens[cu[b]] if n > 0 else np.zeros(tokens.shape[1]) for b, n in enumerate(lens)])
    return O.cross_encoder_logit(w, cls[:, None, :])


# ---- MODEL_ERR: rounded_forward's maximum per-token relative error against the oracle on the inputs of the GPU tests -------------------
# (geometry name, layers) -> (value, the inputs it is the maximum over).  Recomputed by tools in test_anybert_cpu.py (TINY, ODD, BASE at 2
# layers must reproduce to 10 %).  The GPU bars are 2 x these: the ratio the tuned path's token bar (2e-2) has to its model's maximum (1.0e-2).
def model_inputs(name, layers):
    if (name, layers) == ("BASE", 12):
        return [synth_set(5, 256)]
    if (name, layers) == ("LARGE", 4):
        return [synth_set(3, 512)]
    return [edge_tokens(), synth_set(9, 40)]


SHARP = dict(scale=4.0, seed=3)      # "TINY_SHARP": TINY with Linear weights four times as large -- attention that is not nearly uniform


def model_weights(name, layers, head=False):
    """the weights MODEL_ERR[name, layers] was measured on"""
    if name == "TINY_SHARP":
        return TINY, make_weights(TINY, layers, head=head, **SHARP)
    return GEOMS[name], make_weights(GEOMS[name], layers, seed=0, head=head)


def measure_model_err(name, layers):
    geom, w = model_weights(name, layers)
    worst = 0.0
    for ids, tt, lens in model_inputs(name, layers):
        ref = oracle_tokens(w, ids, tt, lens, geom, layers)
        worst = max(worst, float(rel_err(rounded_forward(w, ids, tt, lens, geom, layers), ref).max()))
    return worst


MODEL_ERR = {
    ("TINY", 2): 6.91e-3,
    ("ODD", 2): 6.58e-3,
    ("SMALL", 2): 5.94e-3,
    ("BASE", 2): 5.92e-3,
    ("LARGE", 2): 6.00e-3,
    ("BASE", 12): 1.29e-2,          # synth_set(5, 256)
    ("LARGE", 4): 7.96e-3,          # synth_set(3, 512)
    ("TINY_SHARP", 2): 7.63e-3,     # the weights on which a wrong softmax scale shows (test_anybert_cpu.py: test_the_bars_discriminate)
}
