"""The wide exact scan's regimes and its bit-level reference, guarded without a GPU.

tests/wide_regimes.py restates the planner of `scan_wide_kernel` (rmu_wide_plan, the WCfg table and its LDS terms, pad_dim, deep_bounds)
and lists the corpora and cases that tests/test_wide_regimes_gpu.py holds the kernel to.  Here:
  * every restated constant is read back out of scan_wide.hip / rmu_api.hip / rmu.h and must equal it;
  * the planner's invariants hold for every nq 1..300, k in {1, 32, 33, 112} and n around every multiple of 32 up to 70 000;
  * the cases reach every configuration (with variant_cases() the two plain forms), 1, 2 and 3 tiles per workgroup, both block-map
    branches, 1..4 query tiles of w2_k1 and every nq / k boundary from both sides;
  * the C chain and the numpy chain agree bit for bit at the widths 832 and 3072, and every corpus has the property it was built for,
    on the chain scores (on reduced row counts where that changes nothing about what is established);
  * the pin bites on ties: in every flood case the reference's k-th and (k+1)-th entries have the same score bits and different rows, so
    an answer that breaks ties by the higher row differs from it.
"""
import os
import re
import zlib

import numpy as np
import pytest

from tests import exact_regimes as E
from tests import merge_regimes as M
from tests import wide_regimes as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_STALE = "the wide scan's planner moved: update tests/wide_regimes.py and its GPU cases (tests/test_wide_regimes_gpu.py)"


def _read(rel):
    with open(os.path.join(ROOT, rel), encoding="utf-8") as f:
        return re.sub(r"\s+", " ", f.read())


def _wide():
    return _read("ragmeup_amd/csrc/scan_wide.hip")


def _api():
    return _read("ragmeup_amd/csrc/rmu_api.hip")


def _header():
    return _read("include/rmu.h")


_WQ = r"p->wq = p->kv == 1 \? (\d+) : \(p->nq <= (\d+) \? 1 : \(p->nq <= (\d+) \? 2 : 4\)\);"
_DPAD = r"if \(p->dpad < (\d+) \|\| p->dpad > RMU_MAX_DIM_WIDE \|\| p->dpad % (\d+) != 0\) return RMU_E_INVALID;"
_PAD_DIM = (r"static int pad_dim\(int d\) \{ return d <= 192 \? 192 : \(d <= 384 \? 384 : \(d <= RMU_MAX_DIM \? 768 : "
            r"\(d <= RMU_MAX_DIM_WIDE \? \(d \+ (\d+)\) / (\d+) \* (\d+) : -1\)\)\); \}")
_DEEP_LOOP = r"for \(int64_t c = n / ratio / (\d+) \* (\d+); c >= first && b\.size\(\) < (\d+); c = c / ratio / (\d+) \* (\d+)\) b\.insert\(b\.begin\(\), c\);"
_ROWS = {"w4_k0": (4, 0, 0), "w2_k0": (2, 0, 0), "w1_k0": (1, 0, 0), "w2_k0_nt": (2, 0, 1), "w1_k0_nt": (1, 0, 1), "w2_k1": (2, 1, 0)}      # name -> (wq, kv, NT)


def _cfg_row(name):
    return r"using W_%s = WCfg<(\d+), (\d+), (\d+), (\d+), (\d+), (\d+)>;" % name


# name -> (where, pattern, group, restated value)
SOURCE_CONSTANTS = {
    "kv: k <= 32": (_wide, r"p->kv = p->k <= (\d+) \? 0 : 1;", 1, W.K_SPLIT),
    "wq: kv == 1 -> 2": (_wide, _WQ, 1, W.KV1_WQ),
    "wq: nq <= 32": (_wide, _WQ, 2, W.NQ_W1),
    "wq: nq <= 64": (_wide, _WQ, 3, W.NQ_W2),
    "dpad >= 64": (_wide, _DPAD, 1, W.DPAD_MIN),
    "dpad % 32": (_wide, _DPAD, 2, W.DPAD_STEP),
    "RMU_MAX_K": (_header, r"#define RMU_MAX_K (\d+) ", 1, W.MAX_K),
    "RMU_MAX_DIM": (_header, r"#define RMU_MAX_DIM (\d+) ", 1, W.MAX_DIM),
    "RMU_MAX_DIM_WIDE": (_header, r"#define RMU_MAX_DIM_WIDE (\d+) ", 1, W.MAX_DIM_WIDE),
    "pad_dim: d + 63": (_api, _PAD_DIM, 1, W.PAD_TO - 1),
    "pad_dim: / 64": (_api, _PAD_DIM, 2, W.PAD_TO),
    "pad_dim: * 64": (_api, _PAD_DIM, 3, W.PAD_TO),
    "WCfg: counts 4 * 32 * 4": (_wide, r"THR_OFF = CNT_OFF \+ (\d+) \* (\d+) \* (\d+);", (1, 2, 3), W.LDS_CNT),
    "WCfg: thresholds 4 * 32 * 4": (_wide, r"TRASH_OFF = THR_OFF \+ (\d+) \* (\d+) \* (\d+);", (1, 2, 3), W.LDS_THR),
    "WCfg: trash 256 * 8": (_wide, r"GT_OFF = TRASH_OFF \+ (\d+) \* (\d+);", (1, 2), W.LDS_TRASH),
    "WCfg: shared-threshold landing zone 4 * 256": (_wide, r"LDS_BYTES = GT_OFF \+ (\d+) \* (\d+);", (1, 2), W.LDS_GT),
    "WCfg: the LDS limit": (_wide, r'static_assert\(LDS_BYTES <= (\d+) \* (\d+), "LDS"\);', (1, 2), W.LDS_LIMIT),
    "deep_applies: k > 32": (_api, r"return !off && k > (\d+) && idx->n >= (\d+);", 1, W.DEEP_K),
    "deep_applies: n >= 262144": (_api, r"return !off && k > (\d+) && idx->n >= (\d+);", 2, W.DEEP_N),
    "deep_bounds: RMU_DEEP_FIRST": (_api, r'static const int first = rmu_env\("RMU_DEEP_FIRST"\) \? atoi\(rmu_env\("RMU_DEEP_FIRST"\)\) : (\d+);', 1, W.DEEP_FIRST),
    "deep_bounds: RMU_DEEP_RATIO": (_api, r'static const int ratio = rmu_env\("RMU_DEEP_RATIO"\) \? atoi\(rmu_env\("RMU_DEEP_RATIO"\)\) : (\d+);', 1, W.DEEP_RATIO),
    "deep_bounds: levels": (_api, _DEEP_LOOP, 3, W.DEEP_LEVELS),
}
for _g in (1, 2, 4, 5):
    SOURCE_CONSTANTS[f"deep_bounds: whole 128-row units ({_g})"] = (_api, _DEEP_LOOP, _g, W.DEEP_ALIGN)
for _name, (_wq, _kv, _nt) in _ROWS.items():
    SOURCE_CONSTANTS[f"WCfg row W_{_name}: WQ"] = (_wide, _cfg_row(_name), 1, _wq)
    for _g, _what in enumerate(("CKF", "RING", "CAP", "NCHECK")):
        SOURCE_CONSTANTS[f"WCfg row W_{_name}: {_what}"] = (_wide, _cfg_row(_name), _g + 2, W.WCFG[(_wq, _kv)][_g])
    SOURCE_CONSTANTS[f"WCfg row W_{_name}: NT"] = (_wide, _cfg_row(_name), 6, _nt)

# structural facts the restatement relies on (no number to compare: the pattern must simply be there)
SOURCE_SHAPES = {
    "the planner routes dpad > 768 and RMU_OPT_WIDE_SCAN here": (lambda: _read("ragmeup_amd/csrc/scan_topk.hip"),
                                                                 r"if \(p->wide \|\| p->dpad > RMU_MAX_DIM\) return rmu_wide_plan\(p\);"),
    "rows per tile: 32 * (4 / wq)": (_wide, r"const int rt = 32 \* \(4 / p->wq\);"),
    "query tiles": (_wide, r"p->nqt = \(p->nq \+ 32 \* p->wq - 1\) / \(32 \* p->wq\);"),
    "chunks from the planner": (_wide, r"rmu_plan_chunks\(p->nqt, \(p->n_rows \+ rt - 1\) / rt, &p->s_chunks, &p->tiles_per_chunk\);"),
    "grid and parts": (_wide, r"p->grid = p->s_chunks \* p->nqt; p->parts = p->s_chunks \* \(4 / p->wq\);"),
    "nt: RMU_NT, one query tile, k <= 32, wq <= 2": (_wide, r"p->nt = \(nt_env && p->nqt == 1 && p->kv == 0 && p->wq <= 2\) \? 1 : 0;"),
    "RMU_NT defaults to 1": (_wide, r'static const int nt_env = rmu_env\("RMU_NT"\) \? atoi\(rmu_env\("RMU_NT"\)\) : 1;'),
    "RMU_NO_SHARED_THR clears share_thr": (_api, r'static const int share = rmu_env\("RMU_NO_SHARED_THR"\) \? 0 : 1;'),
    "LDS bytes are the configuration's": (_wide, r"p->lds_bytes = with_wcfg\(p->wq, p->kv, 0, \[\]\(auto c\) \{ return \(int\)decltype\(c\)::LDS_BYTES; \}\);"),
    "with_wcfg": (_wide, r"switch \(wq \* 2 \+ kv\) \{ case 8: return f\(W_w4_k0\{\}\); case 4: return nt \? f\(W_w2_k0_nt\{\}\) : f\(W_w2_k0\{\}\); "
                         r"case 2: return nt \? f\(W_w1_k0_nt\{\}\) : f\(W_w1_k0\{\}\); case 5: return f\(W_w2_k1\{\}\); default: return RMU_E_INVALID; \}"),
    "WCfg: RT = 32 * (4 / WQ), NQ = 32 * WQ": (_wide, r"RP = 4 / WQ_;.*RT = 32 \* RP;.*NQ = 32 \* WQ_;"),
    "WCfg: a slot holds the rows' and the queries' chunk": (_wide, r"SLOT_BYTES = \(RT \+ NQ\) \* CKF_ \* 4;"),
    "WCfg: ring = RING * slot": (_wide, r"RING_BYTES = RING_ \* SLOT_BYTES;"),
    "WCfg: candidates 4 * 32 * CAP * 8": (_wide, r"CAND_BYTES = 4 \* 32 \* CAP_ \* 8; static constexpr int CNT_OFF = RING_BYTES \+ CAND_BYTES;"),
    "WCfg: A = 32 / NCHECK": (_wide, r"A = 32 / NCHECK_;"),
    "chunks per tile: dpad / CKF": (_wide, r"const int nch = dpad / C::CKF;"),
    "the chain: four MFMAs per K-step, x y z w": (_wide, r"acc = __builtin_amdgcn_mfma_f32_32x32x2f32\(av\[t\]\.x, bv\[t\]\.x, acc, 0, 0, 0\);.*av\[t\]\.y, bv\[t\]\.y.*av\[t\]\.z, bv\[t\]\.z.*av\[t\]\.w, bv\[t\]\.w"),
    "the key normalises -0.0": (_wide, r"rmu_make_key\(acc\[r\] \+ 0\.0f,"),
    "the filter passes v >= shared bound": (_wide, r"thr_g = \(go && a\.share_thr\) \? rmu_ord2f\(go - 1u\) : -INFINITY;"),
    "dim == dpad: rows are copied in one piece": (_api, r"if \(idx->dpad == idx->dim\) RMU_HIP_TRY\(hipMemcpyAsync\(dst, vecs,"),
    "deep_bounds ends at n": (_api, r"std::vector<int64_t> b\{n\};"),
}


def _value(m, group):
    if isinstance(group, tuple):
        return int(np.prod([int(m.group(g)) for g in group]))
    return int(m.group(group))


@pytest.mark.parametrize("name", list(SOURCE_CONSTANTS))
def test_restated_constant_equals_the_source(name):
    where, pat, group, restated = SOURCE_CONSTANTS[name]
    m = re.search(pat, where())
    assert m, f"{name}: not found in the source any more -- {_STALE}"
    assert _value(m, group) == restated, f"{name}: the source says {_value(m, group)}, tests/wide_regimes.py says {restated} -- {_STALE}"


@pytest.mark.parametrize("name", list(SOURCE_SHAPES))
def test_restated_structure_is_in_the_source(name):
    where, pat = SOURCE_SHAPES[name]
    assert re.search(pat, where()), f"{name}: not found in the source any more -- {_STALE}"


def test_the_dispatch_table_has_no_row_the_restatement_lacks():
    assert sorted(re.findall(r"using W_(\w+) = WCfg<", _wide())) == sorted(_ROWS)
    assert set(W.CONFIGS) | set(W.PLAIN_CONFIGS) == set(_ROWS)


def test_pad_dim_gives_the_wide_widths():
    assert {d: W.pad_dim(d) for d in W.WIDE_DIMS} == W.WIDE_DIMS
    assert all(W.pad_dim(d) == p for d, p in E.DIMS.items()) and W.pad_dim(3073) == -1 and W.pad_dim(768) == 768 and W.pad_dim(769) == 832
    assert {W.plan_wide(1, 1, 1, 832)["nch"], W.plan_wide(1, 1, 33, 832)["nch"]} == {26, 52}
    assert {W.plan_wide(1, 1, 1, 3072)["nch"], W.plan_wide(1, 1, 33, 3072)["nch"]} == {96, 192}
    assert W.deep_bounds(W.LADDER_N) == [16_384, 65_536, W.LADDER_N]


def test_lds_bytes_against_the_static_limit():
    seen = {}
    for nq, k in ((32, 32), (64, 32), (128, 32), (1, 33), (256, 112)):
        for dpad in sorted(set(W.WIDE_DIMS.values())) + list(E.WIDTHS):
            p = W.plan_wide(10_000, nq, k, dpad)
            ckf, ring, cap, ncheck = W.WCFG[(p["wq"], p["kv"])]
            assert p["lds_bytes"] <= W.LDS_LIMIT and dpad % ckf == 0 and p["A"] == 32 // ncheck
            assert (W.K_SPLIT if p["kv"] == 0 else W.MAX_K) + p["A"] <= cap           # k + A <= CAP: the slot-overflow boundary
            seen[p["config"]] = p["lds_bytes"]
    assert seen == {"w1_k0_nt": 131_072, "w2_k0_nt": 118_784, "w4_k0": 131_072, "w2_k1": 151_552}
    assert W.plan_wide(1, 1, 112, 832)["CAP"] == 112 + W.plan_wide(1, 1, 112, 832)["A"] == 120        # met exactly at k = 112: 112 kept + 8 free


# ---- planner invariants ---------------------------------------------------------------------------------------------------------------
def test_chunks_partition_the_tiles_and_the_merge_accepts_the_parts():
    merge_parts = max(c.parts for c in M.CASES)               # the merge kernels are pinned up to this many part lists
    assert merge_parts == 1040 and W.MAX_K <= M.MAX_K
    shapes = {}
    for nq in range(1, 301):
        for k in (1, 32, 33, 112):
            p = W.plan_wide(0, nq, k, 832)
            shapes.setdefault((p["RT"], p["nqt"], p["wq"]), (nq, k))
            assert p["nqt"] * 32 * p["wq"] >= nq > (p["nqt"] - 1) * 32 * p["wq"]
            assert p["wq"] == 2 if k > W.K_SPLIT else p["wq"] == (1 if nq <= 32 else 2 if nq <= 64 else 4)
    assert set(shapes) == {(128, 1, 1), (64, 1, 2), (32, 1, 4), (32, 2, 4), (32, 3, 4), (64, 2, 2), (64, 3, 2), (64, 4, 2), (64, 5, 2)}
    n_arr = np.array(sorted({v for m in range(0, 70_000, 32) for v in (m - 1, m, m + 1) if v >= 0}), np.int64)
    for (rt, nqt, wq), (nq, k) in shapes.items():
        for t in np.unique((n_arr + rt - 1) // rt):
            s, tpc = W.plan_chunks(nqt, int(t))
            assert 1 <= s <= 256 and tpc >= 1, (rt, nqt, t)
            if t > 0:
                assert (s - 1) * tpc < t <= s * tpc, f"tiles {t}, nqt {nqt}: {s} chunks of {tpc} leave an empty chunk or lose tiles"
            assert s * (4 // wq) <= merge_parts
    for c in W.CASES + W.NARROW_CASES + W.variant_cases():
        for nt_env in (0, 1):
            p = W.plan_wide(c.n, c.nq, c.k, c.dpad, nt_env)
            assert p["parts"] <= merge_parts and p["parts"] * c.k < 2 ** 32 and p["grid"] == p["s_chunks"] * p["nqt"] and p["lds_bytes"] <= W.LDS_LIMIT
            assert 0 < p["tiles_last_chunk"] <= p["tiles_per_chunk"] and (p["s_chunks"] - 1) * p["tiles_per_chunk"] + p["tiles_last_chunk"] == p["tiles_total"]


def test_the_row_counts_of_each_tile_class():
    for rt, nq in ((32, 65), (64, 33), (128, 1)):
        rows = W.class_rows(rt)
        for name, tpc in (("t1_xcd", 1), ("t1_small", 1), ("one", 1), ("few", 1), ("t2", 2), ("t3", 3), ("t3_full", 3)):
            p = W.plan_wide(rows[name], nq, 1, 832)
            assert (p["RT"], p["tiles_per_chunk"]) == (rt, tpc), (rt, name)
        assert rows["t2"] % rt == 1 and rows["t3"] % rt == 1 and rows["t1_xcd"] % rt == 0 and rows["t3_full"] % rt == rt - 1
        assert W.plan_wide(rows["t1_xcd"], nq, 1, 832)["xcd_branch"] and W.plan_wide(rows["t1_xcd"] + 1, nq, 1, 832)["tiles_per_chunk"] == 2
        assert W.plan_wide(rows["t3"] - 2 * rt, nq, 1, 832)["tiles_per_chunk"] == 2
        assert not W.plan_wide(rows["t1_small"], nq, 1, 832)["xcd_branch"] and W.plan_wide(rows["t1_small"], nq, 1, 832)["s_chunks"] == 6
        p = W.plan_wide(rows["t3"], nq, 1, 832)
        assert p["tiles_last_chunk"] < p["tiles_per_chunk"]          # a last chunk with fewer tiles than the others: the clamped tail reloads
    assert [W.class_rows(rt)[name] for rt in (32, 64, 128) for name in ("t2", "t3")] == [8225, 16417, 16449, 32833, 32897, 65665]


# ---- coverage of the cases --------------------------------------------------------------------------------------------------------------
def _ip_random(dim=None):
    return [c for c in W.CASES if c.metric == "ip" and c.corpus == "random" and (dim is None or c.dim == dim)]


def test_cases_reach_every_configuration_tile_class_branch_and_query_tile_count():
    reached = []
    switched = {(c.dim, W.plan_wide(c.n, c.nq, c.k, c.dpad, nt_env=0)["config"], c.plan["tile_class"]) for c in W.variant_cases() if c.corpus == "random"}
    for dim in (769, 1024, 1536, 3072):
        some = _ip_random(dim)
        full = dim in (769, 1024)
        one_tile = {(c.plan["config"], c.plan["tile_class"]) for c in some if c.plan["nqt"] == 1}
        for cfg in W.CONFIGS:
            classes = (1, 2, 3) if full else ((2, 3) if cfg == "w4_k0" else (2,))
            for t in classes:
                assert (cfg, t) in one_tile, f"{cfg} at {dim} dimensions never runs with {t} tiles per workgroup"
                reached.append(f"d{dim} {cfg} x {t} tiles")
        assert {c.plan["nqt"] for c in some if c.plan["config"] == "w2_k1"} == {1, 2, 3, 4}, "query tiles of w2_k1"
        assert {c.plan["nqt"] for c in some if c.plan["config"] == "w4_k0"} == {1, 2}
        reached.append(f"d{dim} w2_k1 x 1..4 query tiles, w4_k0 x 1..2")
        if full:
            branches = {(c.plan["config"], c.plan["xcd_branch"]) for c in some}
            assert branches == {(cfg, b) for cfg in W.CONFIGS for b in (True, False)}, branches
            assert {(c.plan["nqt"] > 1, c.plan["xcd_branch"]) for c in some} == {(a, b) for a in (True, False) for b in (True, False)}
            assert {0, 1} <= {c.n % c.plan["RT"] for c in some} and any(c.n % c.plan["RT"] == c.plan["RT"] - 1 for c in some)
            assert {c.n for c in some} >= {1, 31}
            reached.append(f"d{dim} both block-map branches for every configuration")
    for dim in (769, 3072):                                   # the plain forms: RMU_NT=0 only
        for cfg in W.PLAIN_CONFIGS:
            classes = (2,) if (dim == 3072 and cfg == "w1_k0") else (2, 3)       # 65 665 rows of 3072 floats add no code path
            for t in classes:
                assert (dim, cfg, t) in switched, f"no RMU_NT=0 case runs {cfg} at {dim} dimensions with {t} tiles"
                reached.append(f"d{dim} {cfg} x {t} tiles (RMU_NT=0)")
    assert not {c.plan["config"] for c in W.CASES + W.NARROW_CASES} & set(W.PLAIN_CONFIGS), "the default process cannot reach a plain form"
    for c in W.CASES + W.NARROW_CASES:
        assert c.n < W.DEEP_N and c.n * c.dpad * 4 <= W.CORPUS_BYTES
    print("\n".join(reached))


def test_cases_reach_every_boundary_from_both_sides():
    for dim in (769, 1024, 1536, 3072):
        some = _ip_random(dim)
        k0 = {c.nq for c in some if c.k <= W.K_SPLIT}
        assert k0 >= {1, W.NQ_W1, W.NQ_W1 + 1, W.NQ_W2, W.NQ_W2 + 1, 128, 129, 256}, k0
        assert {c.nq for c in some if c.k > W.K_SPLIT} == {1, 32, 33, 64, 65, 129, 256}
        assert {c.k for c in some} == {1, W.K_SPLIT, W.K_SPLIT + 1, W.MAX_K}
        for nq in (W.NQ_W1, W.NQ_W1 + 1, W.NQ_W2, W.NQ_W2 + 1):          # the boundaries at the deepest class the width runs
            assert any(c.nq == nq and c.k == 32 and c.plan["tile_class"] >= 2 for c in some), nq
    mono = [c for c in W.CASES if c.corpus in ("rising", "falling")]
    for kind in ("rising", "falling"):
        for dim in (769, 3072):
            mine = [c for c in mono if c.corpus == kind and c.dim == dim]
            assert {c.k for c in mine} == {1, 32, 33, 112} and {c.plan["config"] for c in mine} == set(W.CONFIGS)
            assert all(c.plan["tile_class"] == (2 if (dim == 3072 and c.plan["RT"] == 128) else 3) for c in mine)
    for dim in (769, 1024, 1536):
        mine = [c for c in W.CASES if c.metric == "cosine" and c.dim == dim]
        assert {(c.plan["config"], c.plan["tile_class"]) for c in mine} == {("w4_k0", 2), ("w4_k0", 3), ("w2_k1", 3)}
    d1000 = [c for c in W.CASES if c.dim == 1000]
    assert {(c.metric, c.plan["tile_class"]) for c in d1000} == {("cosine", 2), ("cosine", 3), ("ip", 2)}
    var = W.variant_cases()
    assert {c.k for c in var if c.corpus == "rising"} == {32, 112} and {c.plan["RT"] for c in var if c.corpus == "rising"} == {32, 64, 128}
    assert {c.dim for c in var if c.corpus == "rising"} == {769}


def test_the_narrow_corpora_run_through_the_wide_kernel_in_every_configuration():
    fam = W.families(W.NARROW_CASES)
    assert set(fam) == {(100, "random", "ip"), (768, "random", "ip"), (384, "scaled", "cosine")}
    for f, cases in fam.items():
        assert {c.plan["tile_class"] for c in cases} >= {2, 3} and all(c.dpad in E.WIDTHS for c in cases)
    for dim in (100, 768):
        cases = fam[(dim, "random", "ip")]
        assert {c.plan["config"] for c in cases} == set(W.CONFIGS)
        assert {c.plan["RT"] for c in cases if c.plan["tile_class"] >= 2} == {32, 64, 128}
    assert {c.plan["nch"] for c in W.NARROW_CASES} == {6, 12, 24, 48}
    assert {(c.n, c.nq, c.k) for c in W.NARROW_CASES} <= {(c.n, c.nq, c.k) for c in E.CASES}


# ---- the reference at the wide widths -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [769, 3072])
def test_c_chain_equals_numpy_chain_on_a_slice_of_every_corpus(dim):
    dpad = W.WIDE_DIMS[dim]
    for kind in ("random", "scaled", "rising", "falling"):
        x, q = W.corpus(kind, dim, 4000)
        rows = np.r_[0:6, W.flood_layout()[0][2][:3], 3990:3996]
        qs = q[np.r_[0:2, W.ZERO_QUERY:W.ZERO_QUERY + 2]]
        xi, qi = (W.row_norm_image(x[rows], dpad), W.row_norm_image(qs, dpad)) if kind == "scaled" else (x[rows], qs)
        track = {}
        c, p = W.chain(qi, xi, dpad), W.chain_numpy(qi, xi, dpad, track)
        assert np.array_equal(W.bits(c), W.bits(p)), f"the C chain and the numpy chain disagree on {kind}"
        assert track["product"] >= 2.0 ** -126 and track["sum"] >= 2.0 ** -126, f"a subnormal product or partial sum: {track}"
        if kind == "random":                                      # (the corpus of the GPU file's k-order test)
            nat = E.cflat.chain_scores(qi, xi, dpad, natural=True)
            live = np.abs(c) > 0
            assert (W.bits(nat) != W.bits(c))[live].mean() > 0.5, "the natural k order gives the chain's bits: the pin is not order-sensitive"


def test_the_wave_sum_of_squares_at_a_wide_width():
    rng = np.random.default_rng(7)
    v = rng.standard_normal((5, 1000)).astype(np.float32) * np.float32(3.0)
    s = E.cflat.wave_sumsq(W.pad(v, 1024), 1024)
    row = W.pad(v[:1], 1024)[0]
    lanes = np.zeros(64, np.float32)
    for c in range(1024):
        lanes[c % 64] = np.float32(np.float64(row[c]) * np.float64(row[c]) + np.float64(lanes[c % 64]))
    for o in (32, 16, 8, 4, 2, 1):
        lanes = (lanes + lanes[np.arange(64) ^ o]).astype(np.float32)
    assert abs(float(lanes[0]) - float(s[0])) <= 2 * np.spacing(np.float32(s[0]))
    img = W.row_norm_image(v, 1024)
    assert img.shape == (5, 1024) and not img[:, 1000:].any() and np.abs(np.linalg.norm(img.astype(np.float64), axis=1) - 1).max() < 1e-6


# ---- the corpora have the properties they were built for --------------------------------------------------------------------------------
def test_the_flood_sizes_cover_both_wide_slot_depths_and_every_k():
    sizes = set(W.FLOOD_SIZES)
    for cap in {c[2] for c in W.WCFG.values()}:
        assert cap + 1 in sizes and 3 * cap <= max(sizes), cap
    assert {64, 120} == {c[2] for c in W.WCFG.values()} and {65, 121, 192} <= sizes and max(sizes) >= 360
    assert {k + 1 for k in (1, 32, 33, 112)} <= sizes
    lay = W.flood_layout()
    assert len(lay) == 3 * len(W.FLOOD_SIZES) <= W.ZERO_QUERY and {w for _, w, _ in lay} == {"spread", "boundary", "run"}
    assert max(r.max() for _, _, r in lay) < W.FLOOD_END <= W.class_rows(32)["t3"]
    assert len(np.unique(np.concatenate([r for _, _, r in lay]))) == sum(m for m, _, _ in lay)
    # the placements, at the 3-tile row count of every RT (a unit of 384 rows = 4 / 2 / 1 whole chunks there)
    for rt, nq in ((32, 65), (64, 33), (128, 1)):
        p = W.plan_wide(W.class_rows(rt)["t3"], nq, 1, 832)
        chunk = p["RT"] * p["tiles_per_chunk"]
        assert p["tiles_per_chunk"] == 3 and W.UNIT % chunk == 0
        for m, where, rows in lay:
            chunks, tiles = np.unique(rows // chunk), np.unique(rows // rt)
            if where == "run" and m <= rt:
                assert tiles.size == 1, "a run no longer than a tile lies inside one tile"
            if where == "boundary":
                assert tiles.size >= 2 and (m > 65 or chunks.size == 1), "a run across a tile boundary inside one chunk"
            if where == "spread" and m >= 33:
                first = rows[rows // chunk == chunks[0]]
                assert chunks.size >= 3 and first.size < 8 and (first // rt == (chunks[0] + 1) * p["tiles_per_chunk"] - 1).all()


@pytest.mark.parametrize("dim,kind", [(769, "random"), (3072, "random"), (1000, "scaled")])
def test_flood_copies_are_bit_identical_best_rows_and_a_tie_sits_at_every_k(dim, kind):
    """... and the pin bites on ties: where a cluster has more than k copies the reference's k-th and (k+1)-th entries have the same
    score bits and different rows, so a top-k with ties broken by the higher row is another answer."""
    dpad = W.WIDE_DIMS[dim]
    lay = W.flood_layout()
    x, q = W.corpus(kind, dim, W.FLOOD_END)
    qi, xi, _ = E.images("cosine" if kind == "scaled" else "ip", q[:len(lay)], x, dim, dpad)
    s = W.chain(qi, xi, dpad)
    ties = 0
    for i, (m, where, rows) in enumerate(lay):
        assert rows.size == m and len({x[r].tobytes() for r in rows}) == 1
        sb = W.bits(s[i])
        assert len(set(sb[rows].tolist())) == 1, "copies with different score bits"
        assert s[i, rows[0]] > np.delete(s[i], rows).max(), f"cluster {i} is not its query's best"
        for k in (1, 32, 33, 112):
            es, er = W.expected_topk(s[i:i + 1], None, k + 1)
            kk = min(k + 1, m)
            assert np.array_equal(er[0, :kk], rows[:kk]) and (W.bits(es[0, :kk]) == sb[rows[0]]).all()
            if m > k:
                assert W.bits(es)[0, k - 1] == W.bits(es)[0, k] and er[0, k - 1] != er[0, k]
                hi = rows[::-1][:k]                           # the same scores with the HIGHER rows first: not the reference's answer
                assert W.mismatch(es[:, :k], hi[None, :], es[:, :k], er[:, :k])
                ties += 1
    assert ties >= 3 * (len(W.FLOOD_SIZES) + 6 + 4 + 3)           # every cluster at k = 1; 7, 5 and 4 sizes exceed 32, 33 and 112


def test_every_flood_case_has_a_tie_at_its_k():
    """every case over a flood corpus (wide and narrow) has queries whose k-th and (k+1)-th best are copies of one cluster"""
    for c in W.CASES + W.NARROW_CASES:
        if c.corpus in ("random", "scaled") and c.n >= W.FLOOD_END:
            lay = W.flood_layout() if c.dim in W.WIDE_DIMS else E.flood_layout()
            assert any(m > c.k for m, _, _ in lay[:c.nq]), c.id


@pytest.mark.parametrize("dim", [769, 3072])
@pytest.mark.parametrize("kind", ["rising", "falling"])
def test_monotone_corpora_are_strictly_monotone_on_the_chain_scores(kind, dim):
    dpad = W.WIDE_DIMS[dim]
    n = W.rows_max(dpad)
    x, q = W.corpus(kind, dim, n)
    qs = q[np.r_[0:4, 124:132, 252:256]]
    for a in (0, n // 2 - 1500, n - 3000):                     # the steps are smallest, relative to the score, where the scale is largest
        s = W.chain(qs, x[a:a + 3000], dpad)
        d = np.diff(s, axis=1)
        assert (s > 0).all() and ((d > 0) if kind == "rising" else (d < 0)).all(), f"rows {a}..{a + 3000} are not strictly {kind}"


def test_zero_query_expects_the_first_rows_and_zero_bits():
    for dim in (769, 1024):
        x, q = W.corpus("random", dim, 4000)
        assert not q[W.ZERO_QUERY].any()
        s = W.chain(q[W.ZERO_QUERY:W.ZERO_QUERY + 1], x, W.WIDE_DIMS[dim])
        assert (W.bits(s) == 0).all()
        es, er = W.expected_topk(-s, None, 33)                   # (-0.0 scores: normalised as the key does)
        assert (W.bits(es) == 0).all() and np.array_equal(er[0], np.arange(33))


def test_the_narrow_corpora_are_unchanged():
    """the flood sizes are a parameter of exact_regimes.corpus now: its default is the narrow layout, byte for byte"""
    assert E.FLOOD_SIZES == (384, 192, 129, 113, 65, 34, 33, 2)
    assert all(np.array_equal(a[2], b[2]) for a, b in zip(E.flood_layout(), E.flood_layout(E.FLOOD_SIZES)))
    x, q = E.corpus("random", 100, 5000)
    assert (zlib.crc32(x.tobytes()), zlib.crc32(q.tobytes())) == (1138148070, 2316415024)       # as before the parameter existed


def test_the_late_floods_sit_where_the_bound_arrives_first():
    floods = W.late_floods()
    assert len(np.unique(np.concatenate(floods))) == sum(f.size for f in floods) and {W.plan_wide(W.late_rows(rt), nq, k, 832)["config"] for rt, nq, k in W.LATE} == {"w1_k0_nt", "w2_k0_nt", "w4_k0"}
    for (rt, nq, k), rows in zip(W.LATE, floods):
        p = W.plan_wide(W.late_rows(rt), nq, k, W.WIDE_DIMS[W.LATE_DIM])
        assert (p["RT"], p["tiles_per_chunk"], p["nqt"]) == (rt, 5, 1) and p["grid"] <= 256 and W.late_rows(rt) * 832 * 4 <= W.CORPUS_BYTES
        assert W.plan_wide(W.late_rows(rt) - 2 * rt, nq, k, 832)["tiles_per_chunk"] == 4          # the smallest 5-tile count
        tile, few = rows // rt, W.LATE_FEW
        assert (tile[:few] == 5 * (W.LATE_CHUNK + 1) - 1).all(), "the lowest rows: the last tile of their chunk"
        assert sorted(set(tile[few:].tolist())) == [5 * (W.LATE_CHUNK + 2) + t for t in range(3)], "the others: the first three tiles of a later chunk"
        # a wave's slot takes 32 of them per tile and is compacted when it holds more than CAP - A: at the end of the second tile, with k or more
        assert 32 <= p["CAP"] - p["A"] < 64 and k <= 64 and few < k < rows.size and rows.max() < W.late_rows(min(r for r, _, _ in W.LATE))


def test_the_ladder_corpus():
    b = W.deep_bounds(W.LADDER_N)
    assert [c for _, c in W.LADDER_FLOODS] == b[:2] and {m for m, _ in W.LADDER_FLOODS} == {34, 113}
    floods = W.ladder_floods()
    for (m, centre), rows in zip(W.LADDER_FLOODS, floods):
        assert rows.size == m and (rows < centre).sum() >= m // 2 and (rows >= centre).sum() >= m // 2       # copies on both sides of the level's end
    # the third flood, at the geometry of the last level's launch (the same for every k > 32)
    late, start = floods[2], b[-2]
    few, rest, c0 = W.LADDER_LATE
    for k in (33, 112):
        p = W.plan_wide(b[-1] - start, W.LADDER_NQ, k, W.WIDE_DIMS[W.LADDER_DIM])
        chunk, tile = p["RT"] * p["tiles_per_chunk"], (late - start) // p["RT"]
        assert p["config"] == "w2_k1" and p["grid"] <= 256, "one wave of workgroups: the publishing one runs beside the one that waits"
        assert (tile[:few] == (c0 + 1) * p["tiles_per_chunk"] - 1).all(), "the lowest copies: the last tile of their chunk"
        assert ((late[few:] - start) // chunk == c0 + 2).all() and (tile[few:] < (c0 + 2) * p["tiles_per_chunk"] + p["tiles_per_chunk"] // 2).all()
        assert few < k and rest >= 2 * p["CAP"] and late.size > k and late.max() < b[-1] and np.array_equal(late, np.sort(late))
    assert len(np.unique(np.concatenate(floods))) == sum(f.size for f in floods)
