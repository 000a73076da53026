"""CPU: the general encoder (csrc/bert_any.hip: BERTs with 64-wide heads) as far as it can be held without a GPU -- the oracle at head
width 64, rmu_bert_create's argument checks, what ragmeup_amd.checkpoint accepts and refuses, and the error model the GPU bars come from
(tests/anybert.py: rounded_forward, MODEL_ERR)."""
import ctypes
import json
import os
import re
import warnings

import numpy as np
import pytest

from ragmeup_amd import checkpoint as C
from ragmeup_amd.bert import BertCfg, weight_order
from tests import anybert as A
from tests.helpers import write_st_checkpoint


# ---- the oracle at head width 64 ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,layers", [("TINY", 2), ("BASE", 1)])
def test_oracle_matches_transformers_at_head_width_64(name, layers):
    import torch
    from oracle import oracle as O
    geom = A.GEOMS[name]
    w = A.make_weights(geom, layers, seed=2, head=True)
    ids, tt, lens = A.tokens_with_lens([40, 7, 1, 23], seed=3, pair=True)
    ref = O.bert_hidden(w, ids, tt, lens, n_layers=layers, n_heads=geom[1])
    mask = torch.from_numpy((np.arange(ids.shape[1])[None] < lens[:, None]).astype(np.int64))
    ti, tti = torch.from_numpy(ids.astype(np.int64)), torch.from_numpy(tt.astype(np.int64))
    with torch.no_grad():
        enc = A.hf_model({k: v for k, v in w.items() if not k.startswith(("pooler.", "classifier."))}, geom, layers, False)
        hs = enc(input_ids=ti, attention_mask=mask, token_type_ids=tti).last_hidden_state.numpy()
        logit = A.hf_model(w, geom, layers, True)(input_ids=ti, attention_mask=mask, token_type_ids=tti).logits.numpy()[:, 0]
    for b, l in enumerate(lens):
        assert np.abs(hs[b, :l] - ref[b, :l]).max() <= 1e-5
    assert np.abs(O.cross_encoder_logit(w, ref) - logit).max() <= 1e-5


# ---- rmu_bert_create's argument checks (no HIP call is reached) ------------------------------------------------------------
def _create(librmu, hidden, heads, ffn, layers=2, n_weights=None, null_weights=False, has_head=0, max_pos=512):
    cfg = BertCfg(1000, hidden, layers, heads, ffn, max_pos, 2, 1e-12, has_head)
    need = 5 + 16 * layers + (4 if has_head else 0)
    n = need if n_weights is None else n_weights
    ptrs = (ctypes.c_void_p * max(n, 1))(*[None if null_weights else 0x1000] * max(n, 1))
    h = ctypes.c_void_p()
    rc = librmu.rmu_bert_create(ctypes.byref(h), ctypes.byref(cfg), ptrs, n)
    return rc, librmu.rmu_last_error().decode()


def test_create_accepts_general_geometries_up_to_the_weight_count(librmu):
    """cfg BASE with a wrong tensor count is refused for the COUNT: the geometry check has let it through."""
    for geom in (A.BASE, A.LARGE, A.TINY, A.ODD, (1024, 16, 64)):
        rc, msg = _create(librmu, *geom, n_weights=7)
        assert rc == -1 and "wrong number of weight tensors" in msg, (geom, msg)
        rc, msg = _create(librmu, *geom, null_weights=True)
        assert rc == -1 and "null weight pointer" in msg, (geom, msg)
    rc, msg = _create(librmu, *A.BASE, max_pos=513, n_weights=7)
    assert rc == -1 and "max_pos" in msg                      # the order of the checks: geometry, max_pos, count, pointers


@pytest.mark.parametrize("hidden,heads,ffn", [(768, 10, 3072), (1088, 17, 4352), (768, 12, 4160), (768, 12, 100), (384, 8, 1536), (64, 1, 256),
                                              (768, 12, 0)])
def test_create_still_refuses_everything_else(librmu, hidden, heads, ffn):
    rc, msg = _create(librmu, hidden, heads, ffn, n_weights=7)
    assert rc == -1 and "this build supports hidden 384, 12 heads, ffn 1536" in msg and "64-wide heads" in msg, msg
    rc, msg = _create(librmu, *A.BASE, layers=49, n_weights=7)
    assert rc == -1 and "this build supports" in msg


def test_create_tuned_geometry_behaves_as_before(librmu):
    rc, msg = _create(librmu, 384, 12, 1536, layers=6, n_weights=100)
    assert rc == -1 and "wrong number of weight tensors" in msg
    rc, msg = _create(librmu, 384, 12, 1536, layers=6, null_weights=True)
    assert rc == -1 and "null weight pointer" in msg
    assert librmu.rmu_bert_create(None, None, None, 0) == -1 and b"null argument" in librmu.rmu_last_error()


def test_no_new_kernel_spills_to_scratch(librmu, tmp_path):
    """every kernel of bert_any.hip, not only the one whose name the existing scratch test matches"""
    import shutil
    import subprocess
    from ragmeup_amd import _native
    objdump, readelf = "/opt/rocm/lib/llvm/bin/llvm-objdump", "/opt/rocm/lib/llvm/bin/llvm-readelf"
    if not (os.path.exists(objdump) and os.path.exists(readelf)):
        pytest.skip("ROCm's llvm-objdump / llvm-readelf are not installed")
    so = tmp_path / "librmu.so"
    shutil.copy(_native.SO_PATH, so)
    assert subprocess.run([objdump, "--offloading", str(so)], capture_output=True, text=True, cwd=tmp_path).returncode == 0
    seen = {}
    for co in sorted(tmp_path.glob("librmu.so.*gfx950")):
        notes = subprocess.run([readelf, "--notes", str(co)], capture_output=True, text=True).stdout
        for name, scratch in re.findall(r"\.name:\s+(\S+)\n\s+\.private_segment_fixed_size:\s+(\d+)", notes):
            if re.search(r"k_any_|k_gemm_any", name):
                seen[name] = int(scratch)
    assert len(seen) >= 11, sorted(seen)                       # 8 kernels + the GEMM's three epilogues
    assert not {n: s for n, s in seen.items() if s}, seen


# ---- checkpoint directories ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["BASE", "LARGE", "TINY"])
def test_general_checkpoint_directories_are_read(tmp_path, name):
    geom = A.GEOMS[name]
    d = str(tmp_path / name)
    A.write_dir(d, geom, layers=1)
    s = C.read_sentence_transformer(d)
    assert (s.arch.hidden, s.arch.heads, s.arch.ffn, s.arch.layers) == (*geom, 1)
    assert (s.pooling, s.normalize, s.max_seq_length) == ("mean", True, 512)
    state = C.load_state(s)
    assert state["embeddings.word_embeddings.weight"].shape[1] == geom[0]
    ce = str(tmp_path / (name + "_ce"))
    A.write_dir(ce, geom, layers=1, head=True)
    s = C.read_cross_encoder(ce)
    assert s.arch.hidden == geom[0] and s.arch.num_labels == 1 and s.activation == "sigmoid"


def test_geometries_outside_both_paths_are_refused_by_name(tmp_path):
    for geom in ((768, 10, 3072), (1088, 17, 4352), (768, 12, 4160), (384, 8, 1536), (768, 12, 100)):
        with pytest.raises(C.UnsupportedCheckpoint, match="384/12/1536") as e:
            C.read_arch({"num_hidden_layers": 2, "num_attention_heads": geom[1], "hidden_size": geom[0], "intermediate_size": geom[2], "vocab_size": 10})
        assert "64-wide heads" in str(e.value)
    with pytest.raises(C.UnsupportedCheckpoint, match="num_hidden_layers"):
        C.read_arch({"num_hidden_layers": 49, "num_attention_heads": 12, "hidden_size": 768, "intermediate_size": 3072, "vocab_size": 10})


def test_a_config_that_contradicts_the_stored_tensors_is_refused(tmp_path):
    """config.json edited to 768/12/3072 over 384-wide tensors (test_checkpoint_cpu.py's case, which used to be refused as a geometry):
    an inconsistent directory, refused for that, ahead of the pooling-dimension check -- and the same for a .bin, once it is loaded."""
    d = str(tmp_path / "edited")
    write_st_checkpoint(d, layers=1)
    p = os.path.join(d, "config.json")
    c = json.load(open(p))
    c.update(hidden_size=768, intermediate_size=3072)
    json.dump(c, open(p, "w"))
    with pytest.raises(C.UnsupportedCheckpoint, match=r"declares hidden/heads/ffn = 768/12/3072 but the stored tensors are those of 384/12/1536"):
        C.read_sentence_transformer(d)
    with pytest.raises(C.UnsupportedCheckpoint, match="stored tensors"):
        C._common(d)
    b = str(tmp_path / "edited_bin")
    A.write_dir(b, A.TINY, layers=1, binfile=True)
    p = os.path.join(b, "config.json")
    c = json.load(open(p))
    c.update(hidden_size=768, num_attention_heads=12, intermediate_size=3072)
    json.dump(c, open(p, "w"))
    json.dump({"word_embedding_dimension": 768, "pooling_mode_cls_token": False, "pooling_mode_mean_tokens": True},
              open(os.path.join(b, "1_Pooling", "config.json"), "w"))
    spec = C.read_sentence_transformer(b)                     # (nothing of a pickle is read to describe it)
    with pytest.raises(C.UnsupportedCheckpoint, match=r"768/12/3072 but the stored tensors are those of 128/12/512"):
        C.load_state(spec)
    ok = str(tmp_path / "bin_ok")
    A.write_dir(ok, A.TINY, layers=1, binfile=True)
    assert set(C.load_state(C.read_sentence_transformer(ok))) >= set(weight_order(1, False))


def test_no_gpu_no_encoder(monkeypatch):
    import torch
    from ragmeup_amd.bert import BertEncoder
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        BertEncoder(A.make_weights(A.BASE, 1), layers=1, heads=12, ffn=3072)


# ---- the error model ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def edge_refs():
    """(weights, EDGE tokens, oracle rows) per geometry name, computed once"""
    cache = {}

    def get(name):
        if name not in cache:
            geom, w = A.model_weights(name, A.LAYERS)
            ids, tt, lens = A.edge_tokens()
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                cache[name] = (geom, w, (ids, tt, lens), A.oracle_tokens(w, ids, tt, lens, geom))
        return cache[name]
    return get


def test_rounding_model_without_rounding_is_the_oracle(edge_refs):
    geom, w, (ids, tt, lens), ref = edge_refs("TINY")
    assert ref.shape == (sum(A.EDGE_LENS), geom[0])
    assert A.rel_err(A.rounded_forward(w, ids, tt, lens, geom, rounding=False), ref).max() < 1e-9
    x = np.array([1.0, 1.00390625, 1.01171875, -1.0048828125, 0.0], np.float32)       # ties go to even mantissas
    assert A.bf16_round(x).tolist() == [1.0, 1.0, 1.015625, -1.0078125, 0.0]


@pytest.mark.parametrize("name", ["TINY", "ODD", "BASE", "TINY_SHARP"])
def test_model_err_table_is_what_the_model_gives(name):
    got = A.measure_model_err(name, A.LAYERS)
    print(f"MODEL_ERR[{name}, {A.LAYERS}]: stored {A.MODEL_ERR[name, A.LAYERS]:.4e}, recomputed {got:.4e}")
    assert abs(got - A.MODEL_ERR[name, A.LAYERS]) <= 0.1 * got


def test_model_err_table_covers_every_gpu_case():
    assert set(A.MODEL_ERR) == {(n, A.LAYERS) for n in A.GEOMS} | {("BASE", 12), ("LARGE", 4), ("TINY_SHARP", A.LAYERS)}
    assert all(3e-3 < v < 2e-2 for v in A.MODEL_ERR.values())      # bf16 has 8 bits: a few 2^-9 steps per value, a dozen rounding points deep


@pytest.mark.parametrize("name", ["TINY", "ODD", "BASE"])
@pytest.mark.parametrize("mutation", A.MUTATIONS)
def test_the_bars_discriminate(edge_refs, name, mutation):
    """Each wrong forward must miss the GPU bar, 2 x MODEL_ERR, on EDGE.  Four of the five do on the standard weights.  The fifth, a softmax
    scale of 1/sqrt(32), does NOT there (measured: 6.7e-3 at TINY and ODD against bars of 1.4e-2 and 1.3e-2, 1.8e-2 at BASE against 1.2e-2):
    with Linear weights of N(0, 0.02) the scores are so small that attention is nearly uniform whatever the scale -- the bar is too loose for
    that mistake on those weights.  The narrower check is TINY_SHARP, the same geometry with weights four times as large (scores that
    matter): there the wrong scale gives 1.1e-1 against a bar of 1.5e-2, and the GPU tests run those weights as a case of their own."""
    geom, w, (ids, tt, lens), ref = edge_refs(name)
    err = float(A.rel_err(A.rounded_forward(w, ids, tt, lens, geom, mutate=mutation), ref).max())
    bar = 2 * A.MODEL_ERR[name, A.LAYERS]
    print(f"{name} {mutation}: {err:.3e} against the bar {bar:.3e}")
    if mutation == "scale32":
        geom, w, (ids, tt, lens), ref = edge_refs("TINY_SHARP")
        err = float(A.rel_err(A.rounded_forward(w, ids, tt, lens, geom, mutate=mutation), ref).max())
        bar = 2 * A.MODEL_ERR["TINY_SHARP", A.LAYERS]
        print(f"TINY_SHARP {mutation}: {err:.3e} against the bar {bar:.3e}")
    assert err > bar
