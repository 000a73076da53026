"""The encoder's dispatch table, guarded without a GPU.

tests/encoder_regimes.py restates `enqueue_forward`'s kernel choice (ragmeup_amd/csrc/bert.hip); the GPU file
tests/test_encoder_regimes_gpu.py holds every regime from both sides of each threshold.  Here:
  * every threshold is read back out of bert.hip / bert.py and must equal the restated constant -- a rework that moves one fails
    here, naming it, and the GPU boundary cases have to follow it;
  * CASES must reach every distinct regime() value, and every threshold from both sides (the value itself and the next one up,
    with the regime field the threshold controls differing between them).
"""
import os
import re
import types

import pytest

from tests import encoder_regimes as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _read(rel):
    with open(os.path.join(ROOT, rel), encoding="utf-8") as f:
        return f.read()


def _release_only(src: str) -> str:
    """The source as a build without RMU_DEBUG_KERNELS sees it (the #ifdef blocks of bert.hip do not nest)."""
    out, state = [], None
    for line in src.splitlines():
        t = line.strip()
        if t.startswith("#ifdef RMU_DEBUG_KERNELS"):
            state = "debug"
            continue
        if state and t.startswith("#else"):
            state = "release"
            continue
        if state and t.startswith("#endif"):
            state = None
            continue
        if state != "debug":
            out.append(line)
    return "\n".join(out)


def _forward_body() -> str:
    src = _release_only(_read("ragmeup_amd/csrc/bert.hip"))
    i = src.index("static void enqueue_forward(")
    j = src.index('extern "C" int rmu_bert_encode(', i)
    return re.sub(r"\s+", " ", src[i:j])


def _g3_min_body() -> str:
    src = _release_only(_read("ragmeup_amd/csrc/bert.hip"))
    i = src.index("static int64_t g3_min_tokens()")
    return re.sub(r"\s+", " ", src[i:src.index("}", i) + 1])


def _hip() -> str:
    return re.sub(r"\s+", " ", _read("ragmeup_amd/csrc/bert.hip"))


# name -> (where, pattern with one integer group; evaluated on whitespace-normalised text)
SOURCE_THRESHOLDS = {
    "SMALL_M": (_hip, r"constexpr int SMALL_M = (\d+);"),
    "SMALL_M (g3_min_tokens)": (_g3_min_body, r"return (SMALL_M|\d+); \}"),
    "QKV_ATTN_TOKENS": (_hip, r"constexpr int QKV_ATTN_TOKENS = (\d+),"),
    "QKV_ATTN_MIN_TOKENS": (_hip, r"QKV_ATTN_MIN_TOKENS = (\d+);"),
    "FOLD_TOKENS": (_hip, r"constexpr int FOLD_TOKENS = (\d+);"),
    "FOLD_MAX_LEN": (_forward_body, r"if \(cap <= fold_tokens && max_len <= (\d+) &&"),
    "CU_HERE_BATCH": (_forward_body, r"const bool cu_here = small_fuse && batch <= (\d+) && cap <= FOLD_TOKENS;"),
    "EMBED_SEQ_BATCH": (_forward_body, r"if \(embed_seq && batch >= (\d+)\)"),
    "KT4_MAX_LEN (small, fused)": (_forward_body, r"if \(max_len <= (\d+)\) \{ if \(!prev\) launch_qkv_attn_small<4, false>"),
    "KT4_MAX_LEN (small, two launches)": (_forward_body, r"if \(max_len <= (\d+)\) launch_attn3<4>\(batch, m->qkv, m->cu, m->ctx, false, 0, s\);"),
    "KT4_MAX_LEN": (_forward_body, r"if \(max_len <= (\d+)\) launch_attn3<4>\(batch, m->qkv, m->cu, m->ctx, ctx_tiled"),
    "KT8_MAX_LEN": (_forward_body, r"else if \(max_len <= (\d+)\) launch_attn3<8>\(batch, m->qkv, m->cu, m->ctx, ctx_tiled, hm_stride, s\); "
                                   r"else launch_attn3<16>"),
    "FFN3_TOKENS": (_forward_body, r"const bool fused_ffn = !\(g3_mask & 4\) && \(fused_env < 0 \? cap > (\d+) :"),
    "CTX_TILED_TOKENS": (_forward_body, r"const bool ctx_tiled = tiled_env && attn_v == 3 && !\(g3_mask & 2\) && cap > (\d+);"),
    "HOST_TOKENS": (_hip, r"static constexpr int HOST_TOKENS = (\d+);"),
    "HOST_ROWS": (_hip, r"\(kind == RMU_BERT_TOKENS \? cap : \(int64_t\)batch\) > (\d+)\)"),
    "HOST_TOKENS (bert.py)": (lambda: _read("ragmeup_amd/bert.py"), r"HOST_TOKENS = (\d+)"),
    "HOST_ROWS (bert.py)": (lambda: _read("ragmeup_amd/bert.py"), r"HOST_ROWS = (\d+)"),
}

# structural facts the restated table relies on (no number to compare: the pattern must simply be there)
SOURCE_SHAPES = {
    "fused QKV + attention for QKV_ATTN_MIN_TOKENS < cap <= QKV_ATTN_TOKENS": (_forward_body,
        r"qa_tokens = rmu_env\(\"RMU_QKV_ATTN_TOKENS\"\) \? [^;]* : QKV_ATTN_TOKENS;.*qa_min = rmu_env\(\"RMU_QKV_ATTN_MIN\"\) \? [^;]* : "
        r"QKV_ATTN_MIN_TOKENS;.*if \(cap <= qa_tokens && cap > qa_min\)"),
    "small path up to FOLD_TOKENS": (_forward_body, r"fold_tokens = rmu_env\(\"RMU_FOLD_TOKENS\"\) \? [^;]* : FOLD_TOKENS;"),
    "bulk QKV: k_gemm3 above g3_min_tokens()": (_forward_body,
        r"else if \(\(g3_mask & 1\) && cap > g3_min_tokens\(\)\) launch_gemm3<EPI_BIAS>.* else launch_gemm<EPI_BIAS>"),
    "h tiled between layers only (never out of the last one)": (_forward_body,
        r"const bool h_out_tiled = h_env && ffn_v == 3 && ctx_tiled && \(g3_mask & 1\) && li < m->layers.size\(\);"),
}

_STALE = "the encoder's dispatch moved: update tests/encoder_regimes.py and its GPU boundary cases (tests/test_encoder_regimes_gpu.py)"


@pytest.mark.parametrize("name", list(SOURCE_THRESHOLDS))
def test_threshold_matches_the_source(name):
    where, pat = SOURCE_THRESHOLDS[name]
    m = re.search(pat, where())
    assert m, f"{name}: pattern not found in the source -- {_STALE}"
    const = name.split(" ")[0]
    want = getattr(R, const)
    got = m.group(1)
    got = getattr(R, got) if got.isidentifier() else int(got)
    assert got == want, f"{name}: the source says {got}, tests/encoder_regimes.py says {want} -- {_STALE}"


@pytest.mark.parametrize("name", list(SOURCE_SHAPES))
def test_dispatch_shape_matches_the_source(name):
    where, pat = SOURCE_SHAPES[name]
    assert re.search(pat, where()), f"{name}: not found in the source -- {_STALE}"


def _domain():
    # every regime is reachable at batch <= 640, max_len <= 512 (the thresholds on batch stop at 512, max_pos is 512);
    # layers 1 and 6 (any layers >= 2 gives the values of 6)
    for layers in (1, 6):
        for b in range(1, 641):
            for L in range(1, 513):
                yield b, L, layers


def test_cases_reach_every_regime():
    reach = {}
    for b, L, layers in _domain():
        reach.setdefault(R.encoder_regime(b, L, layers), (b, L, layers))
    covered = {R.encoder_regime(c.batch, c.max_len, c.layers) for c in R.CASES}
    missing = [(v, dict(k)) for k, v in reach.items() if k not in covered]
    assert not missing, f"regimes no GPU case reaches (example shape, regime): {missing}"
    assert covered <= set(reach), "a case's regime lies outside the enumerated domain"


def _var(c, var):
    return {"cap": c.cap, "batch": c.batch, "max_len": c.max_len}[var]


@pytest.mark.parametrize("name,var,t,field", R.THRESHOLDS, ids=[t[0] for t in R.THRESHOLDS])
def test_cases_hold_each_threshold_from_both_sides(name, var, t, field):
    lo = [c for c in R.CASES if _var(c, var) == t]
    hi = [c for c in R.CASES if _var(c, var) == t + 1]
    assert lo and hi, f"{name}: no GPU case at {var} = {t} and {t + 1}"
    pairs = [(a.id, b.id) for a in lo for b in hi
             if R.regime(a.batch, a.max_len, a.layers)[field] != R.regime(b.batch, b.max_len, b.layers)[field]]
    assert pairs, f"{name}: the cases at {var} = {t} / {t + 1} do not differ in {field}"


def test_case_ids_name_their_regime():
    ids = [c.id for c in R.CASES]
    assert len(ids) == len(set(ids))
    for c in R.CASES:
        r = R.regime(c.batch, c.max_len, c.layers)
        assert c.id.startswith("layers") or c.id.split("-")[0].startswith(r["path"]), (c.id, r)
        assert ("tiled" in c.id) == r["ctx_tiled"], (c.id, r)
        assert f"kt{r['attn_kt']}" in c.id or "kt" not in c.id, (c.id, r)
        assert c.layers == 6 or c.id.startswith(f"layers{c.layers}-"), c.id
        assert c.id.endswith(f"-{c.batch}x{c.max_len}"), c.id
        assert c.max_len <= 512 and 1 <= c.batch <= 65535
        if c.lens == "groups":
            assert sum(n for n, _ in c.real) <= c.batch and all(1 <= l <= c.max_len for _, l in c.real), c.id


def test_host_cases_cross_the_fold_threshold():
    """The host entry point pads a call to a bucketed (bb, lb): the host cases land on both sides of FOLD_TOKENS and on
    HOST_TOKENS itself, and one token more is refused."""
    from ragmeup_amd.bert import BertEncoder
    fake = types.SimpleNamespace(max_pos=512, HOST_TOKENS=BertEncoder.HOST_TOKENS, HOST_ROWS=BertEncoder.HOST_ROWS,
                                 _bucket=BertEncoder._bucket)
    caps = []
    for b, L in R.HOST_CASES:
        bb, lb = BertEncoder.host_shape(fake, b, L, R.MODE_MEAN)
        assert bb >= b and lb >= L
        caps.append(bb * lb)
    assert min(caps) <= R.FOLD_TOKENS < max(caps) and max(caps) == R.HOST_TOKENS, caps
    assert {R.regime(*BertEncoder.host_shape(fake, b, L, R.MODE_MEAN))["path"] for b, L in R.HOST_CASES} == {"small", "bulk"}
    assert BertEncoder.host_shape(fake, 17, 256, R.MODE_MEAN) is None          # 17 x 256 = 4352 tokens
