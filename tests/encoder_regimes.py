"""The encoder's dispatch table (`enc_plan` in ragmeup_amd/csrc/bert_plan.h, launched by `enqueue_forward` in bert.hip), restated
in Python, and the GPU cases that pin each of its regimes from both sides of every threshold.

`regime(batch, max_len, layers, mode)` names the kernels a default build launches for one `rmu_bert_encode` call.  It is a
plain helper module, not a fixture: tests/test_encoder_regimes_cpu.py calls the library's own `enc_plan` (through the internal
export `rmu_bert_plan_`) for every shape of the domain and requires it to equal regime() field by field, compares the constants
below with those of the same name in bert_plan.h / bert.py, and checks that CASES covers every regime and every threshold;
tests/test_encoder_regimes_gpu.py runs CASES against the fp64 oracle.  A rework that moves a threshold, or combines two of them
differently, makes the CPU test fail first: the boundary cases below are then stale.
"""
from __future__ import annotations

from dataclasses import dataclass

MODE_MEAN, MODE_CE, MODE_CLS, MODE_TOKENS = 0, 1, 2, 3      # include/rmu.h RMU_BERT_*
NO_NORMALIZE = 0x100
HIDDEN = 384

# ---- thresholds (tokens = batch * max_len unless named otherwise) ------------------------------------------------------------
SMALL_M = 256                 # bulk QKV projection: k_gemm3 above, k_gemm at or below
QKV_ATTN_TOKENS = 2560        # small path: QKV projection + attention fused (k_qkv_attn_small) for
QKV_ATTN_MIN_TOKENS = 128     #   QKV_ATTN_MIN_TOKENS < cap <= QKV_ATTN_TOKENS
FOLD_TOKENS = 2560            # small (folded-LayerNorm) path up to this cap ...
FOLD_MAX_LEN = 256            # ... and this max_len
CU_HERE_BATCH = 256           # sequence offsets inside k_embed_ln<true> for batch <= this (and cap <= FOLD_TOKENS)
EMBED_SEQ_BATCH = 512         # k_embed_ln_seq (a workgroup per sequence) for batch >= this
KT4_MAX_LEN = 128             # attention tile count KT: 4 up to this max_len,
KT8_MAX_LEN = 256             #   8 up to this one, 16 above (bulk only; the small path stops at FOLD_MAX_LEN)
FFN3_TOKENS = 16384           # k_ffn3 (fused FFN) for cap above this; the GEMM pair + k_layernorm at or below
CTX_TILED_TOKENS = 32768      # ctx written tiled (and h tiled between layers) for cap above this
HOST_TOKENS = 4096            # host entry point (rmu_bert_encode_host): bucketed batch * max_len it accepts
HOST_ROWS = 256               # ... and the result rows


def regime(batch: int, max_len: int, layers: int = 6, mode: int = MODE_MEAN) -> dict:
    """The kernels enqueue_forward launches for this call shape (default build, no RMU_* switches)."""
    cap = batch * max_len
    cu_here = batch <= CU_HERE_BATCH and cap <= FOLD_TOKENS
    if cu_here:
        embed = "k_embed_ln<true>"
    elif batch >= EMBED_SEQ_BATCH:
        embed = "k_embed_ln_seq"
    else:
        embed = "k_embed_ln<false>"
    r = {"embed": embed, "offsets": "k_embed_ln<true>" if cu_here else "k_cu_seqlens"}
    if cap <= FOLD_TOKENS and max_len <= FOLD_MAX_LEN:
        fused = QKV_ATTN_MIN_TOKENS < cap <= QKV_ATTN_TOKENS
        r.update(path="small", qkv="k_qkv_attn_small" if fused else "k_gemm_small", qkv_attn_fused=fused,
                 attn_kt=4 if max_len <= KT4_MAX_LEN else 8, ffn="k_gemm_small", ctx_tiled=False, h_tiled=False)
    else:
        ctx_tiled = cap > CTX_TILED_TOKENS
        r.update(path="bulk", qkv="k_gemm3" if cap > SMALL_M else "k_gemm", qkv_attn_fused=False,
                 attn_kt=4 if max_len <= KT4_MAX_LEN else 8 if max_len <= KT8_MAX_LEN else 16,
                 ffn="k_ffn3" if cap > FFN3_TOKENS else "k_gemm+k_layernorm", ctx_tiled=ctx_tiled,
                 h_tiled=ctx_tiled and layers > 1)        # the last layer writes h row-major: one layer never tiles it
    kind = mode & 0xff
    r["head"] = {MODE_MEAN: "k_pool", MODE_CLS: "k_pool", MODE_TOKENS: "k_tokens_out", MODE_CE: "k_cls_head"}[kind]
    return r


def encoder_regime(batch: int, max_len: int, layers: int = 6) -> tuple:
    """regime() without the output head, as a hashable value"""
    r = regime(batch, max_len, layers)
    r.pop("head")
    return tuple(sorted(r.items()))


# ---- the GPU cases ----------------------------------------------------------------------------------------------------------
# lens kinds (tests/test_encoder_regimes_gpu.py builds them, seeded by the case id):
#   "ramp"   random lengths in [1, max_len] with the longest (max_len) and the shortest (1) present
#   "full"   every sequence max_len long
#   "groups" `real` lists (count, length) groups, spread over the batch by a seeded permutation; the rest of the batch is empty
@dataclass(frozen=True)
class Case:
    id: str
    batch: int
    max_len: int
    layers: int = 6
    lens: str = "ramp"
    real: tuple = ()

    @property
    def cap(self) -> int:
        return self.batch * self.max_len


CASES = [
    # small path, QKV projection and attention as two launches (cap <= 128)
    Case("small2-len1-1x1", 1, 1, lens="full"),
    Case("small2-len2-1x2", 1, 2, lens="full"),
    Case("small2-cap128-1x128", 1, 128, lens="full"),
    Case("small2-cap128-2x64", 2, 64),
    # small path, fused k_qkv_attn_small (128 < cap <= 2560)
    Case("small-fused-cap129-3x43", 3, 43),
    Case("small-fused-kt8-cap256-1x256", 1, 256, lens="full"),
    Case("small-fused-kt4-len128-10x128", 10, 128),
    Case("small-fused-kt8-len129-10x129", 10, 129),
    Case("small-fused-kt4-cap2560-20x128", 20, 128),
    Case("small-fused-kt8-cap2560-10x256", 10, 256),
    # batch boundaries with short sequences
    Case("small-cuhere-batch256-256x8", 256, 8),
    Case("small-cuseq-batch257-257x8", 257, 8),
    Case("small-cuseq-batch511-511x4", 511, 4),
    Case("small-embedseq-batch512-512x4", 512, 4),
    Case("small-embedseq-len1-2000x1", 2000, 1, lens="full"),
    # bulk from cap 2561, and because max_len > 256 at a small cap
    Case("bulk-cap2561-kt8-13x197", 13, 197),
    Case("bulk-len257-kt16-1x257", 1, 257, lens="full"),
    Case("bulk-len512-kt16-1x512", 1, 512, lens="full"),
    Case("bulk-pair-kt16-cuhere-8x320", 8, 320),
    Case("bulk-pair-kt16-8x400", 8, 400),
    # GEMM pair vs fused FFN; KT 4 vs 8 inside the GEMM-pair regime
    Case("bulk-pair-cap16384-kt4-128x128", 128, 128),
    Case("bulk-pair-kt8-len129-127x129", 127, 129),
    Case("bulk-ffn3-cap16385-kt4-145x113", 145, 113),
    Case("bulk-ffn3-kt16-60x300", 60, 300),
    # row-major vs tiled ctx / h
    Case("bulk-ffn3-cap32768-kt8-128x256", 128, 256),
    Case("bulk-tiled-cap32769-kt16-99x331", 99, 331),
    Case("bulk-tiled-kt4-300x128", 300, 128),
    # padding-heavy tiled batches: fewer real tokens than one 16-token block / just over one 128-token tile
    Case("bulk-tiled-sparse15-129x256", 129, 256, lens="groups", real=((5, 3),)),
    Case("bulk-tiled-sparse131-200x256", 200, 256, lens="groups", real=((10, 13), (1, 1))),
    # bulk at batch >= 512 (k_embed_ln_seq)
    Case("bulk-embedseq-pair-kt4-512x6", 512, 6),
    Case("bulk-embedseq-ffn3-kt4-512x40", 512, 40),
    Case("bulk-embedseq-tiled-kt4-600x64", 600, 64),
    Case("bulk-embedseq-tiled-kt8-512x160", 512, 160, lens="groups", real=((64, 150), (448, 9))),
    Case("bulk-embedseq-tiled-kt16-512x300", 512, 300, lens="groups", real=((32, 290), (480, 7))),
    # models of 1 and 2 layers: the first layer is the last one (h never tiled at 1 layer)
    Case("layers1-small-fused-12x100", 12, 100, layers=1),
    Case("layers1-tiled-kt8-130x256", 130, 256, layers=1),
    Case("layers1-tiled-kt4-257x128", 257, 128, layers=1),
    Case("layers1-tiled-kt16-65x505", 65, 505, layers=1),
    Case("layers1-embedseq-tiled-kt4-512x65", 512, 65, layers=1),
    Case("layers1-embedseq-tiled-kt8-512x129", 512, 129, layers=1),
    Case("layers1-embedseq-tiled-kt16-512x257", 512, 257, layers=1, lens="groups", real=((16, 257), (496, 5))),
    Case("layers2-small-fused-12x100", 12, 100, layers=2),
    Case("layers2-tiled-kt8-130x256", 130, 256, layers=2),
]

# (threshold name, the variable it tests, the last value on its lower side, the regime field it switches)
THRESHOLDS = [
    ("QKV_ATTN_MIN_TOKENS", "cap", QKV_ATTN_MIN_TOKENS, "qkv_attn_fused"),
    ("QKV_ATTN_TOKENS", "cap", QKV_ATTN_TOKENS, "qkv_attn_fused"),
    ("FOLD_TOKENS", "cap", FOLD_TOKENS, "path"),
    ("FOLD_MAX_LEN", "max_len", FOLD_MAX_LEN, "path"),
    ("SMALL_M", "cap", SMALL_M, "qkv"),
    ("CU_HERE_BATCH", "batch", CU_HERE_BATCH, "offsets"),
    ("EMBED_SEQ_BATCH", "batch", EMBED_SEQ_BATCH - 1, "embed"),     # (batch >= 512: the two sides are 511 and 512)
    ("KT4_MAX_LEN", "max_len", KT4_MAX_LEN, "attn_kt"),
    ("KT8_MAX_LEN", "max_len", KT8_MAX_LEN, "attn_kt"),
    ("FFN3_TOKENS", "cap", FFN3_TOKENS, "ffn"),
    ("CTX_TILED_TOKENS", "cap", CTX_TILED_TOKENS, "ctx_tiled"),
]

# host entry point (rmu_bert_encode_host through BertEncoder.encode_host): input (batch, max_len); BertEncoder.host_shape buckets
# them to (1, 32) 32, (12, 128) 1536, (24, 128) 3072, (12, 256) 3072 and (16, 256) 4096 tokens -- both sides of FOLD_TOKENS
HOST_CASES = [(1, 30), (9, 100), (20, 120), (10, 250), (16, 256)]
