"""The encoder's dispatch table, guarded without a GPU.

tests/encoder_regimes.py restates the encoder's kernel choice; the GPU file tests/test_encoder_regimes_gpu.py holds every regime
from both sides of each threshold.  The choice itself is `enc_plan` in ragmeup_amd/csrc/bert_plan.h, a pure function that
`enqueue_forward` (bert.hip) launches and that librmu.so exports for this file as `rmu_bert_plan_`.  Here:
  * the plan must EQUAL the restated table for every shape of the domain (batch 1-640 x max_len 1-512, 1 and 6 layers) -- behaviour,
    not the spelling of a condition: a rework that moves a threshold or combines two of them differently fails here, and the GPU
    boundary cases have to follow it;
  * every threshold constant of the restated table equals the one of the same name in bert_plan.h (bert.py's two as well);
  * every RMU_* environment set the GPU variant tests run still selects something: it changes the plan, and only behind RMU_TUNING=1;
  * CASES must reach every distinct regime() value, and every threshold from both sides (the value itself and the next one up,
    with the regime field the threshold controls differing between them).
"""
import ast
import ctypes
import os
import re
import subprocess
import sys
import types

import numpy as np
import pytest

from tests import encoder_regimes as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _read(rel):
    with open(os.path.join(ROOT, rel), encoding="utf-8") as f:
        return f.read()


_STALE = "the encoder's dispatch moved: update tests/encoder_regimes.py and its GPU boundary cases (tests/test_encoder_regimes_gpu.py)"

# ---- the numbers -----------------------------------------------------------------------------------------------------------
HEADER_NAMES = ["SMALL_M", "QKV_ATTN_TOKENS", "QKV_ATTN_MIN_TOKENS", "FOLD_TOKENS", "FOLD_MAX_LEN", "CU_HERE_BATCH", "EMBED_SEQ_BATCH",
                "KT4_MAX_LEN", "KT8_MAX_LEN", "FFN3_TOKENS", "CTX_TILED_TOKENS", "HOST_TOKENS", "HOST_ROWS"]
# name -> (file, pattern with one integer group): one uniform pattern for the header, bert.py's class attributes
SOURCE_THRESHOLDS = {n: ("ragmeup_amd/csrc/bert_plan.h", rf"constexpr int {n} = (\d+);") for n in HEADER_NAMES}
SOURCE_THRESHOLDS["HOST_TOKENS (bert.py)"] = ("ragmeup_amd/bert.py", r"HOST_TOKENS = (\d+)")
SOURCE_THRESHOLDS["HOST_ROWS (bert.py)"] = ("ragmeup_amd/bert.py", r"HOST_ROWS = (\d+)")


@pytest.mark.parametrize("name", list(SOURCE_THRESHOLDS))
def test_threshold_matches_the_source(name):
    rel, pat = SOURCE_THRESHOLDS[name]
    m = re.search(pat, _read(rel))
    assert m, f"{name}: not found in {rel} -- {_STALE}"
    want = getattr(R, name.split(" ")[0])
    assert int(m.group(1)) == want, f"{name}: {rel} says {m.group(1)}, tests/encoder_regimes.py says {want} -- {_STALE}"


# ---- the plan --------------------------------------------------------------------------------------------------------------
# EncPlan as rmu_bert_plan_ writes it out (bert_plan.h documents the order next to the struct)
FIELDS = ("offsets_fused", "embed", "path", "qkv", "attn_kt", "gemm", "out_proj", "ffn", "ffn_ln_in", "ctx_tiled", "h_tiled",
          "qkv_head_major", "tq", "th", "tf")
QKV_KERNEL = {"GemmSmall": "k_gemm_small", "AttnSmall": "k_qkv_attn_small", "Gemm": "k_gemm", "Gemm3": "k_gemm3", "Qa": "k_qa"}
FFN_KERNEL = {"GemmSmall": "k_gemm_small", "PairLn": "k_gemm+k_layernorm", "Gemm3Pair": "k_gemm3+k_layernorm", "Ffn2": "k_ffn2",
              "Ffn3": "k_ffn3"}


def _header_enums():
    """enum class NAME : int32_t { A, B, ... } of bert_plan.h -> {NAME: [A, B, ...]} (the enumerators count from 0)"""
    h = _read("ragmeup_amd/csrc/bert_plan.h")
    enums = {n: [e.strip() for e in body.split(",")] for n, body in re.findall(r"enum class (\w+) : int32_t \{([^}]*)\}", h)}
    assert int(re.search(r"constexpr int ENC_PLAN_FIELDS = (\d+);", h).group(1)) == len(FIELDS)
    assert all(f in h[h.index("struct EncPlan {"):] for f in FIELDS)
    return enums


def _plan_fn(lib):
    fn = lib.rmu_bert_plan_            # internal symbol: not in _native's list, so it is declared here
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int]
    return fn


def _as_regime(row, enums):
    """one plan (a sequence of len(FIELDS) ints) in regime()'s words"""
    p = dict(zip(FIELDS, row))
    qkv, gemm = enums["EncQkv"][p["qkv"]], enums["EncGemm"][p["gemm"]]
    return {"embed": "k_embed_ln<true>" if p["offsets_fused"] else {"Wave": "k_embed_ln<false>", "Seq": "k_embed_ln_seq"}[enums["EncEmbed"][p["embed"]]],
            "offsets": "k_embed_ln<true>" if p["offsets_fused"] else "k_cu_seqlens",
            "path": enums["EncPath"][p["path"]].lower(),
            "qkv": "k_gemm_small" if (qkv, gemm) == ("Gemm", "Small") else QKV_KERNEL[qkv],      # (launch_gemm's own small form)
            "qkv_attn_fused": qkv == "AttnSmall", "attn_kt": p["attn_kt"], "ffn": FFN_KERNEL[enums["EncFfn"][p["ffn"]]],
            "ctx_tiled": bool(p["ctx_tiled"]), "h_tiled": bool(p["h_tiled"])}


REGIME_FIELDS = ("embed", "offsets", "path", "qkv", "qkv_attn_fused", "attn_kt", "ffn", "ctx_tiled", "h_tiled")


def _domain():
    # every regime is reachable at batch <= 640, max_len <= 512 (the thresholds on batch stop at 512, max_pos is 512);
    # layers 1 and 6 (any layers >= 2 gives the values of 6)
    for layers in (1, 6):
        for b in range(1, 641):
            for L in range(1, 513):
                yield b, L, layers


def test_plan_equals_the_restated_table(librmu):
    """enc_plan (what enqueue_forward launches) against regime() (what the GPU cases are built on), field by field, over the whole
    domain -- and at 2 layers on the shapes of CASES.  One call sweeps max_len 1..512 for a (batch, layers)."""
    enums, plan = _header_enums(), _plan_fn(librmu)
    nf = len(FIELDS)
    buf = np.full((512, nf), -1, dtype=np.int32)
    said = {}                              # the plan's regime-relevant fields -> regime()'s words for them (a few dozen distinct rows)
    wrong = []
    for layers in (1, 6):
        for b in range(1, 641):
            assert plan(b, 1, layers, buf.ctypes.data, buf.size) == 512
            for L, row in enumerate(map(tuple, buf[:, :12].tolist()), start=1):
                got = said.get(row) or said.setdefault(row, _as_regime(row, enums))
                want = R.regime(b, L, layers)
                if any(got[f] != want[f] for f in REGIME_FIELDS) and len(wrong) < 5:
                    wrong.append(((b, L, layers), {f: (got[f], want[f]) for f in REGIME_FIELDS if got[f] != want[f]}))
    for c in R.CASES:
        one = np.zeros(nf, dtype=np.int32)
        assert plan(c.batch, c.max_len, 2, one.ctypes.data, nf) == 1
        got, want = _as_regime(one.tolist(), enums), R.regime(c.batch, c.max_len, 2)
        if any(got[f] != want[f] for f in REGIME_FIELDS):
            wrong.append(((c.batch, c.max_len, 2), {f: (got[f], want[f]) for f in REGIME_FIELDS if got[f] != want[f]}))
    assert not wrong, f"(shape, field: (plan, restated table)) {wrong} -- {_STALE}"


# ---- the switches ----------------------------------------------------------------------------------------------------------
def _variant_envs():
    """The environment sets tests/test_encoder_gpu.py runs the kernel variants under: the parametrisation of its variant test, read
    from its source (importing it would import torch), plus RMU_QA 0 / 1 of its k_qa test."""
    tree = ast.parse(_read("tests/test_encoder_gpu.py"))
    fn = next(n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "test_every_switchable_kernel_variant_keeps_parity")
    sets = next(ast.literal_eval(d.args[1]) for d in fn.decorator_list
                if isinstance(d, ast.Call) and isinstance(d.args[0], ast.Constant) and d.args[0].value == "env")
    assert len(sets) == 12, sets
    return sets + [e for e in ({"RMU_QA": "1"}, {"RMU_QA": "0"}) if e not in sets]


_PRINT_PLANS = """
import ctypes, sys
import numpy as np
lib = ctypes.CDLL(sys.argv[1])
lib.rmu_bert_plan_.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_int]
out = []
for batch, max_len in ((300, 250), (3, 40)):
    p = np.zeros(int(sys.argv[2]), dtype=np.int32)
    assert lib.rmu_bert_plan_(batch, max_len, 6, p.ctypes.data, p.size) == 1
    out += p.tolist()
print("PLANS", *out)
"""


def _child_plans(env, tuning=True):
    """the plans at 300 x 250 (bulk, everything tiled) and 3 x 40 (small) as a fresh process with this environment sees them"""
    from ragmeup_amd import _native
    base = {k: v for k, v in os.environ.items() if not k.startswith("RMU_")}
    if tuning:
        base["RMU_TUNING"] = "1"
    r = subprocess.run([sys.executable, "-c", _PRINT_PLANS, _native.SO_PATH, str(len(FIELDS))], env=dict(base, **env), capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return next(ln for ln in r.stdout.splitlines() if ln.startswith("PLANS "))


def test_switches_still_steer_the_plan(librmu):
    """The switches are read once per process, so each environment set gets a fresh child.  Every set of the GPU variant tests must
    change at least one field of the plan at 300 x 250 or at 3 x 40 -- a switch that silently stops selecting anything fails here, not
    only where a GPU is -- and without RMU_TUNING none of them may.  RMU_QA=0 spells out that switch's default: it is held to the
    default plan, and RMU_QA=1 to a different one."""
    default = _child_plans({})
    envs = _variant_envs()
    dead = [e for e in envs if e != {"RMU_QA": "0"} and _child_plans(e) == default]
    assert not dead, f"environment sets that no longer change the plan: {dead}"
    assert _child_plans({"RMU_QA": "0"}) == default != _child_plans({"RMU_QA": "1"})
    everything = {k: v for e in envs for k, v in e.items()}
    assert _child_plans(everything, tuning=False) == default, "a switch is honoured without RMU_TUNING=1"


# ---- the cases -------------------------------------------------------------------------------------------------------------
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
