"""The exact fp32 scan's regimes and its bit-level reference, guarded without a GPU.

tests/exact_regimes.py restates the planner of `scan_topk_kernel` (rmu_scan_plan, rmu_plan_chunks, the Cfg table, ScanGeom's LDS terms),
the kernel's arithmetic as an fmaf chain and the corpora that drive its selection machinery; tests/test_exact_regimes_gpu.py holds the
kernel to them.  Here:
  * every restated constant is read back out of scan_topk.hip / scan_common.h / rmu_common.h / rmu.h and must equal it -- a rework that
    moves a threshold or a Cfg row fails here, naming it, and the GPU cases have to follow;
  * the planner's invariants hold for every nq 1..300, k in {1, 32, 33, 112} and n around every multiple of 32 up to 140 000;
  * CASES reaches every (width, configuration), every tile class per RT, both block-map branches with one and two query tiles and
    every nq / k boundary from both sides;
  * the C chain and the numpy chain agree bit for bit (neither is trusted alone), the natural-order chain does NOT (the pin is
    order-sensitive), and every corpus has the property it was built for, on the chain scores.
"""
import os
import re

import numpy as np
import pytest

from tests import exact_regimes as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_STALE = "the exact scan's planner moved: update tests/exact_regimes.py and its GPU cases (tests/test_exact_regimes_gpu.py)"


def _read(rel):
    with open(os.path.join(ROOT, rel), encoding="utf-8") as f:
        return re.sub(r"\s+", " ", f.read())


def _topk():
    return _read("ragmeup_amd/csrc/scan_topk.hip")


def _scan_common():
    return _read("ragmeup_amd/csrc/scan_common.h")


def _common():
    return _read("ragmeup_amd/csrc/rmu_common.h")


def _api():
    return _read("ragmeup_amd/csrc/rmu_api.hip")


def _header():
    return _read("include/rmu.h")


_WQ = r"p->wq = p->nq <= (\d+) \? 1 : \(p->nq <= (\d+) \? 2 : 4\);"
_CHUNK_LOOP = r"for \(int s = (\d+); s <= (\d+); s \+= (\d+)\)"
_EFF = r"const double eff = \(double\)total / \(double\)\(\(\(total \+ (\d+)\) / (\d+)\) \* (\d+)\);"
_DEEP = r"return !off && k > (\d+) && idx->n >= (\d+);"


def _cfg_row(name):
    return r"template <int D> using C_%s = Cfg<D, (\d+), (\d+), (\d+), (\d+), (\d+)(?:, 0, 0)?(?:, 1)?>;" % name


# name -> (where, pattern, group, restated value)
SOURCE_CONSTANTS = {
    "kv: k <= 32": (_topk, r"p->kv = p->k <= (\d+) \? 0 : 1;", 1, E.K_SPLIT),
    "wq: nq <= 32": (_topk, _WQ, 1, E.NQ_W1),
    "wq: nq <= 64": (_topk, _WQ, 2, E.NQ_W2),
    "promotion: kv == 1 && wq == 1 -> 2": (_topk, r"if \(p->kv == 1 && p->wq == 1\) p->wq = (\d+);", 1, E.PROMOTED_WQ),
    "RMU_MAX_K": (_header, r"#define RMU_MAX_K (\d+) ", 1, E.MAX_K),
    "rmu_plan_chunks: first s": (_common, _CHUNK_LOOP, 1, E.CHUNKS_FIRST),
    "rmu_plan_chunks: last s": (_common, _CHUNK_LOOP, 2, E.CHUNKS_LAST),
    "rmu_plan_chunks: step": (_common, _CHUNK_LOOP, 3, E.CHUNKS_STEP),
    "rmu_plan_chunks: round up to 256 (add)": (_common, _EFF, 1, E.CU_ROUND - 1),
    "rmu_plan_chunks: round up to 256 (divide)": (_common, _EFF, 2, E.CU_ROUND),
    "rmu_plan_chunks: round up to 256 (multiply)": (_common, _EFF, 3, E.CU_ROUND),
    "rmu_plan_chunks: stop at total >= 256": (_common, r"if \(total >= (\d+) && eff > 0\.999\) break;", 1, E.CU_ROUND),
    "block_map: s_chunks & 7": (_scan_common, r"if \(\(s_chunks & (\d+)\) == 0\) \{ const int xcd = b & 7, m = b >> 3;", 1, E.XCD_MASK),
    "ScanGeom: counts 4 * 32 * 4": (_scan_common, r"THR_OFF = CNT_OFF \+ (\d+) \* (\d+) \* (\d+);", (1, 2, 3), E.LDS_CNT),
    "ScanGeom: thresholds 4 * 32 * 4": (_scan_common, r"TRASH_OFF = THR_OFF \+ (\d+) \* (\d+) \* (\d+);", (1, 2, 3), E.LDS_THR),
    "ScanGeom: trash 256 * 8": (_scan_common, r"TAIL_OFF = TRASH_OFF \+ (\d+) \* (\d+);", (1, 2), E.LDS_TRASH),
    "Cfg: shared-threshold landing zone 4 * 256": (_topk, r"LDS_BYTES = GT_OFF \+ (\d+) \* (\d+);", (1, 2), E.LDS_GT),
    "deep_applies: k > 32": (_api, _DEEP, 1, E.DEEP_K),
    "deep_applies: n >= 262144": (_api, _DEEP, 2, E.DEEP_N),
}
for _name, _key in (("w4_k0", (4, 0)), ("w4_k1", (4, 1)), ("w2_k0", (2, 0)), ("w2_k1", (2, 1)), ("w1_k0", (1, 0)), ("w2_k0_nt", (2, 0)), ("w1_k0_nt", (1, 0))):
    SOURCE_CONSTANTS[f"Cfg row C_{_name}: WQ"] = (_topk, _cfg_row(_name), 1, _key[0])
    for _g, _what in enumerate(("CKF", "RING", "CAP", "NCHECK")):
        SOURCE_CONSTANTS[f"Cfg row C_{_name}: {_what}"] = (_topk, _cfg_row(_name), _g + 2, E.CFG[_key][_g])

# structural facts the restatement relies on (no number to compare: the pattern must simply be there)
SOURCE_SHAPES = {
    "the widths: 192, 384, 768": (_topk, r"if \(p->dpad != 192 && p->dpad != 384 && p->dpad != 768\) return RMU_E_INVALID;"),
    "rows per tile: 32 * (4 / wq)": (_topk, r"const int rt = 32 \* \(4 / p->wq\);"),
    "query tiles": (_topk, r"p->nqt = \(p->nq \+ 32 \* p->wq - 1\) / \(32 \* p->wq\);"),
    "chunks from the planner": (_topk, r"rmu_plan_chunks\(p->nqt, \(p->n_rows \+ rt - 1\) / rt, &p->s_chunks, &p->tiles_per_chunk\);"),
    "grid and parts": (_topk, r"p->grid = p->s_chunks \* p->nqt; p->parts = p->s_chunks \* \(4 / p->wq\);"),
    "nt: one query tile, k <= 32, wq <= 2": (_topk, r"p->nt = \(nt_env && p->nqt == 1 && p->kv == 0 && p->wq <= 2\) \? 1 : 0;"),
    "RMU_NT defaults to 1": (_topk, r'static const int nt_env = rmu_env\("RMU_NT"\) \? atoi\(rmu_env\("RMU_NT"\)\) : 1;'),
    "RMU_NO_SHARED_THR clears share_thr": (_api, r'static const int share = rmu_env\("RMU_NO_SHARED_THR"\) \? 0 : 1;'),
    "with_cfg: wq * 2 + kv": (_topk, r"switch \(wq \* 2 \+ kv\) \{ case 8: "),
    "with_cfg: w4_k0": (_topk, r"#endif return f\(C_w4_k0<D>\{\}\); \} case 9: return f\(C_w4_k1<D>\{\}\);"),
    "with_cfg: w2": (_topk, r"case 4: return nt \? f\(C_w2_k0_nt<D>\{\}\) : f\(C_w2_k0<D>\{\}\); case 5: return f\(C_w2_k1<D>\{\}\);"),
    "with_cfg: w1": (_topk, r"case 2: return nt \? f\(C_w1_k0_nt<D>\{\}\) : f\(C_w1_k0<D>\{\}\); default: return RMU_E_INVALID;"),
    "the nt rows differ from the plain ones in the last argument only": (_topk,
        r"C_w2_k0 = Cfg<D, 2, 96, 3, 64, 1, 0, 0>;.*C_w1_k0 = Cfg<D, 1, 48, 3, 64, 1, 0, 0>;.*C_w2_k0_nt = Cfg<D, 2, 96, 3, 64, 1, 0, 0, 1>; "
        r"template <int D> using C_w1_k0_nt = Cfg<D, 1, 48, 3, 64, 1, 0, 0, 1>;"),
    "ScanGeom: ring = RING * RT * CKF * 4": (_scan_common, r"SLOT_BYTES = RT \* CKF_ \* 4;.*RING_BYTES = RING_ \* SLOT_BYTES;"),
    "ScanGeom: RT = 32 * (4 / WQ)": (_scan_common, r"RP = 4 / WQ_;.*RT = 32 \* RP;"),
    "ScanGeom: candidates 4 * 32 * CAP * 8": (_scan_common, r"CAND_BYTES = 4 \* 32 \* CAP_ \* 8; static constexpr int CNT_OFF = RING_BYTES \+ CAND_BYTES;"),
    "ScanGeom: A = 32 / NCHECK": (_scan_common, r"A = 32 / NCHECK_;"),
    "Cfg: the landing zone follows ScanGeom's tail": (_topk, r"GT_OFF = G::TAIL_OFF;"),
    "overflow check: count > CAP - A": (_scan_common, r"__ballot\(c > \(u32\)\(C::CAP - C::A\)\)"),
    "rmu_plan_chunks: strictly better efficiency": (_common, r"if \(eff > best_eff \+ 1e-9\) \{ best_eff = eff; best_s = s; \}"),
    "rmu_plan_chunks: fewer tiles than chunks, ceil, trailing chunks dropped": (_common,
        r"if \(tiles_total < s\) s = tiles_total > 0 \? \(int\)tiles_total : 1; \*tiles_per_chunk = \(int\)\(\(tiles_total \+ s - 1\) / s\);.*"
        r"const int64_t used = \(tiles_total \+ \*tiles_per_chunk - 1\) / \*tiles_per_chunk; if \(used > 0 && used < s\) s = \(int\)used;"),
    "the chain's k order": (_topk, r"MFMA number c of // that step multiplies component c, i\.e\. k = 8t\+c \(lanes<32\) and k = 8t\+4\+c \(lanes>=32\)"),
    "the key normalises -0.0": (_topk, r"rmu_make_key\(prev\[r\] \+ 0\.0f,"),
    "the filter passes v >= shared bound": (_topk, r"thr_g = \(go && a\.share_thr\) \? rmu_ord2f\(go - 1u\) : -INFINITY;"),
    "k_row_norm": (_api, r"for \(int c = lane; c < dpad; c \+= 64\) s = fmaf\(row\[c\], row\[c\], s\); #pragma unroll for \(int o = 32; o > 0; o >>= 1\) "
                         r"s \+= __shfl_xor\(s, o\);.*const float inv = 1\.0f / fmaxf\(sqrtf\(s\), 1e-12f\); for \(int c = lane; c < dpad; c \+= 64\) row\[c\] \*= inv;"),
    "k_l2_aug_rows": (_api, r"for \(int c = lane; c < dim; c \+= 64\) s = fmaf\(row\[c\], row\[c\], s\); #pragma unroll for \(int o = 32; o > 0; o >>= 1\) "
                            r"s \+= __shfl_xor\(s, o\); if \(lane == 0\) row\[dim\] = -s;"),
    "k_l2_aug_queries": (_api, r"\{ const float v = row\[c\]; s = fmaf\(v, v, s\); row\[c\] = 2\.0f \* v; \}.*if \(lane == 0\) \{ qn2\[r\] = s; row\[dim\] = 1\.0f; \}"),
    "the merge's L2 step": (lambda: _read("ragmeup_amd/csrc/topk_merge.hip"), r"if \(o\.l2_out\) sc = fmaxf\(o\.qnorm2\[qo\] - sc, 0\.f\);"),
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
    assert _value(m, group) == restated, f"{name}: the source says {_value(m, group)}, tests/exact_regimes.py says {restated} -- {_STALE}"


@pytest.mark.parametrize("name", list(SOURCE_SHAPES))
def test_restated_structure_is_in_the_source(name):
    where, pat = SOURCE_SHAPES[name]
    assert re.search(pat, where()), f"{name}: not found in the source any more -- {_STALE}"


def test_lds_bytes_against_the_static_limit():
    for (wq, kv), (ckf, ring, cap, ncheck) in E.CFG.items():
        for dpad in E.WIDTHS:
            p = E.plan(10_000, {1: 32, 2: 64, 4: 128}[wq], 32 if kv == 0 else 33, dpad)
            assert (p["wq"], p["kv"]) == (wq, kv) and p["lds_bytes"] <= 160 * 1024 and dpad % ckf == 0 and p["A"] == 32 // ncheck
            assert E.K_SPLIT + p["A"] <= cap if kv == 0 else E.MAX_K + p["A"] <= cap          # k + A <= CAP: the slot-overflow boundary
    # the boundary is met exactly at k = 32 and k = 112
    assert E.plan(1, 128, 32, 384)["CAP"] == 32 + E.plan(1, 128, 32, 384)["A"] and E.plan(1, 128, 112, 384)["CAP"] == 112 + E.plan(1, 128, 112, 384)["A"]


# ---- planner invariants ---------------------------------------------------------------------------------------------------------------
def test_chunks_partition_the_tiles():
    ns = sorted({v for m in range(0, 140_000, 32) for v in (m - 1, m, m + 1) if v >= 0})
    shapes = {}
    for nq in range(1, 301):
        for k in (1, 32, 33, 112):
            p = E.plan(0, nq, k, 384)
            shapes.setdefault((p["RT"], p["nqt"], p["wq"]), (nq, k))
    assert set(shapes) == {(128, 1, 1), (64, 1, 2), (32, 1, 4), (32, 2, 4), (32, 3, 4)}       # every (RT, query tiles) of 1..300 queries
    n_arr = np.array(ns, np.int64)
    for (rt, nqt, wq), (nq, k) in shapes.items():
        tiles = (n_arr + rt - 1) // rt
        for t in np.unique(tiles):
            s, tpc = E.plan_chunks(nqt, int(t))
            assert 1 <= s <= 256 and tpc >= 1, (rt, nqt, t)
            if t > 0:
                assert (s - 1) * tpc < t <= s * tpc, f"tiles {t}, nqt {nqt}: {s} chunks of {tpc} leave an empty chunk or lose tiles"
            assert s * (4 // wq) <= 1024
    for nq in range(1, 301):                                    # the per-query-count half: parts and the grid follow the chunks
        for k in (1, 32, 33, 112):
            for n in (1, 31, 4097, 70_001, 139_999):
                p = E.plan(n, nq, k, 768)
                assert p["parts"] <= 1024 and p["grid"] == p["s_chunks"] * p["nqt"] and p["nqt"] * 32 * p["wq"] >= nq > (p["nqt"] - 1) * 32 * p["wq"]
                assert 0 < p["tiles_last_chunk"] <= p["tiles_per_chunk"] and (p["s_chunks"] - 1) * p["tiles_per_chunk"] + p["tiles_last_chunk"] == p["tiles_total"]


def test_the_row_counts_of_each_tile_class():
    for rt, nq in ((32, 65), (64, 33), (128, 1)):
        rows = E.class_rows(rt)
        for name, tpc in (("t2", 2), ("t3", 3), ("t4", 4)):
            n = rows[name]
            assert E.plan(n, nq, 1, 384)["tiles_per_chunk"] == tpc
            assert n % rt == 1                                   # one live row in the last tile
        # 256 tiles still have one each; two tiles less are one tile class less (one live row in the tile behind the first of the class)
        assert E.plan(rows["t1_xcd"], nq, 1, 384)["tiles_per_chunk"] == 1 and E.plan(rows["t1_xcd"] + 1, nq, 1, 384)["tiles_per_chunk"] == 2
        assert E.plan(rows["t3"] - 2 * rt, nq, 1, 384)["tiles_per_chunk"] == 2 and E.plan(rows["t4"] - 2 * rt, nq, 1, 384)["tiles_per_chunk"] == 3
        assert rows["t1_xcd"] % rt == 0 and E.plan(rows["t1_xcd"], nq, 1, 384)["xcd_branch"] and rows["t3_full"] % rt == rt - 1
        for name in ("t3", "t4"):                                # a last chunk with fewer tiles than the others
            p = E.plan(rows[name], nq, 1, 384)
            assert p["tiles_last_chunk"] < p["tiles_per_chunk"]
    assert (E.class_rows(32)["t2"], E.class_rows(32)["t3"], E.class_rows(32)["t4"]) == (8225, 16417, 24609)
    assert (E.class_rows(64)["t2"], E.class_rows(64)["t3"], E.class_rows(64)["t4"]) == (16449, 32833, 49217)
    assert (E.class_rows(128)["t2"], E.class_rows(128)["t3"], E.class_rows(128)["t4"]) == (32897, 65665, 98433)


# ---- coverage of CASES ----------------------------------------------------------------------------------------------------------------
def _ip_random():
    return [c for c in E.CASES if c.metric == "ip" and c.corpus == "random"]


def test_cases_reach_every_width_and_configuration():
    default = {(c.dpad, c.plan["config"]) for c in _ip_random()}
    switched = {(c.dpad, E.plan(c.n, c.nq, c.k, c.dpad, nt_env=0)["config"]) for c in E.variant_cases()}
    for dpad in E.WIDTHS:
        for cfg in E.CONFIGS:
            if cfg in ("w1_k0", "w2_k0"):                        # the plain forms of the non-temporal ones: RMU_NT=0 only
                assert (dpad, cfg) in switched, f"no RMU_NT=0 case runs {cfg} at dpad {dpad}"
            else:
                assert (dpad, cfg) in default, f"no case runs {cfg} at dpad {dpad}"
    assert {c.dim for c in _ip_random() if c.dpad == 768} == {767, 768}


def test_cases_reach_every_tile_class_per_configuration():
    seen = {(c.dpad, c.plan["config"], c.plan["tile_class"]) for c in _ip_random() if c.plan["nqt"] == 1}
    for dpad in E.WIDTHS:
        for cfg in ("w1_k0_nt", "w2_k0_nt", "w2_k1", "w4_k0", "w4_k1"):
            classes = (1, 2) if (dpad == 768 and cfg.startswith("w1")) else (1, 2, 3, 4)    # 98 433 x 768 floats add no code path
            for t in classes:
                assert (dpad, cfg, t) in seen, f"{cfg} at dpad {dpad} never runs with {t} tiles per workgroup"
    for c in E.CASES:
        assert c.n < E.DEEP_N and c.n <= E.rows_max(c.dpad)
    # each deeper class also leaves a last chunk with fewer tiles than the others, a last tile with one live row, n = 0 and n = RT - 1 mod RT
    for dpad in E.WIDTHS:
        some = [c for c in _ip_random() if c.dpad == dpad]
        assert any(c.plan["tiles_last_chunk"] < c.plan["tiles_per_chunk"] for c in some)
        assert {0, 1} <= {c.n % c.plan["RT"] for c in some} and any(c.n % c.plan["RT"] == c.plan["RT"] - 1 for c in some)


def test_cases_reach_both_block_map_branches_with_one_and_two_query_tiles():
    for dpad in E.WIDTHS:
        seen = {(c.plan["nqt"], c.plan["xcd_branch"]) for c in _ip_random() if c.dpad == dpad}
        assert seen >= {(1, True), (1, False), (2, True), (2, False)}, (dpad, seen)
        assert any(c.plan["nqt"] == 2 and c.plan["tiles_per_chunk"] >= 2 for c in _ip_random() if c.dpad == dpad)


def test_cases_reach_every_boundary_from_both_sides():
    for dpad in E.WIDTHS:
        nqs = {c.nq for c in _ip_random() if c.dpad == dpad}
        ks = {c.k for c in _ip_random() if c.dpad == dpad}
        assert nqs >= {1, E.NQ_W1, E.NQ_W1 + 1, E.NQ_W2, E.NQ_W2 + 1, 128, 129}, nqs
        assert ks >= {1, E.K_SPLIT, E.K_SPLIT + 1, E.MAX_K}, ks
        assert any(c.nq <= E.NQ_W1 and c.k > E.K_SPLIT and c.plan["config"] == "w2_k1" for c in _ip_random() if c.dpad == dpad), "the promoted w2_k1"
    mono = [c for c in E.CASES if c.corpus in ("rising", "falling")]
    for kind in ("rising", "falling"):
        for dpad in E.WIDTHS:
            assert {c.k for c in mono if c.corpus == kind and c.dpad == dpad} == {1, 32, 33, 112}
            assert {c.plan["config"] for c in mono if c.corpus == kind and c.dpad == dpad} >= {"w1_k0_nt", "w2_k0_nt", "w2_k1", "w4_k0", "w4_k1"}
    for metric, dims in (("cosine", (100, 384, 768)), ("l2", (100, 383, 767))):
        for dim in dims:
            assert {c.plan["tile_class"] for c in E.CASES if c.metric == metric and c.dim == dim} == {2, 3, 4}
    var = E.variant_cases()
    for dpad in E.WIDTHS:
        seen = {(E.plan(c.n, c.nq, c.k, c.dpad, nt_env=0)["config"], c.plan["tile_class"]) for c in var if c.dpad == dpad and c.corpus == "random"}
        want = {("w2_k0", 2), ("w2_k0", 3), ("w1_k0", 2)} | ({("w1_k0", 3)} if dpad < 768 else set())
        assert seen >= want, (dpad, seen)
    assert {c.k for c in var if c.corpus == "rising"} == {32, 112}


# ---- the reference ------------------------------------------------------------------------------------------------------------------------
def test_round_to_fp32_of_a_rational():
    from fractions import Fraction
    for v in (1.0, 1.0 + 2.0 ** -23, 3.0e-30, -7.25, 2.0 ** 100):
        assert E._round_f32(Fraction(v)) == np.float32(v)
    one, ulp = Fraction(1), Fraction(2) ** -23
    assert E._round_f32(one + ulp / 2) == np.float32(1.0)                          # tie -> even
    assert E._round_f32(one + ulp + ulp / 2) == np.float32(1.0 + 2.0 ** -22)       # tie -> even, upwards
    assert E._round_f32(one + ulp / 2 + Fraction(2) ** -80) == np.float32(1.0 + 2.0 ** -23)
    assert E._round_f32(Fraction(2) - ulp / 4) == np.float32(2.0)                 # carry into the next binade


def test_the_numpy_chain_survives_a_double_rounding():
    """acc = 2^20 + 2^-3 (odd mantissa), product = 2^-4 - 2^-34: the fp64 sum rounds ONTO the fp32 midpoint and ties-to-even would go up;
    the exact sum lies below the midpoint and fmaf keeps acc."""
    x = np.zeros((1, 8), np.float32)
    q = np.zeros((1, 8), np.float32)
    x[0, 0], q[0, 0] = 2.0 ** 20 + 2.0 ** -3, 1.0
    x[0, 4], q[0, 4] = (1.0 + 2.0 ** -15) * 0.25, (1.0 - 2.0 ** -15) * 0.25      # column 4 is the chain's second term
    want = E.bits(np.array([[2.0 ** 20 + 2.0 ** -3]], np.float32))
    naive = (np.float64(x[0, 0]) + np.float64(x[0, 4]) * np.float64(q[0, 4])).astype(np.float32)
    assert E.bits(np.array([[naive]]))[0, 0] != want[0, 0], "the input does not double-round: the test is void"
    assert E.bits(E.chain(q, x, 8))[0, 0] == want[0, 0] and E.bits(E.chain_numpy(q, x, 8))[0, 0] == want[0, 0]


@pytest.mark.parametrize("dim", list(E.DIMS))
def test_c_chain_equals_numpy_chain_and_the_natural_order_does_not(dim):
    dpad = E.DIMS[dim]
    x, q = E.corpus("random", dim)
    rows = np.r_[0:120, E.flood_layout()[0][2][:40], 5000:5140]
    qs = q[np.r_[0:6, E.ZERO_QUERY:E.ZERO_QUERY + 6, 250:256]]
    track = {}
    c, p = E.chain(qs, x[rows], dpad), E.chain_numpy(qs, x[rows], dpad, track)
    assert np.array_equal(E.bits(c), E.bits(p)), "the C chain and the numpy chain disagree"
    assert track["product"] >= 2.0 ** -126 and track["sum"] >= 2.0 ** -126, f"a subnormal product or partial sum: {track}"
    nat = E.cflat.chain_scores(qs, x[rows], dpad, natural=True)
    live = np.abs(c) > 0
    assert (E.bits(nat) != E.bits(c))[live].mean() > 0.5, "the natural k order gives the chain's bits: the pin is not order-sensitive"
    assert np.abs(c.astype(np.float64) - qs.astype(np.float64) @ x[rows].astype(np.float64).T).max() < 1e-5


def test_k_order_is_the_kernel_s():
    ko = E.k_order(16)
    assert ko.tolist() == [0, 4, 1, 5, 2, 6, 3, 7, 8, 12, 9, 13, 10, 14, 11, 15]


def test_no_input_can_make_a_subnormal_product():
    for kind in ("random", "rising", "falling", "scaled"):
        for dim in (100, 768):
            x, q = E.corpus(kind, dim)
            ax, aq = np.abs(x[x != 0]), np.abs(q[q != 0])
            assert float(ax.min()) * float(aq.min()) >= 2.0 ** -126 and float(ax.max()) * float(aq.max()) * E.DIMS[dim] < 1e6


# ---- the corpora have the properties they were built for --------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", list(E.DIMS))
def test_flood_copies_are_bit_identical_best_rows_in_the_intended_places(dim):
    dpad = E.DIMS[dim]
    x, q = E.corpus("random", dim)
    lay = E.flood_layout()
    assert len(lay) <= E.ZERO_QUERY and max(r.max() for _, _, r in lay) < E.FLOOD_END <= E.class_rows(32)["t3"]
    assert len(np.unique(np.concatenate([r for _, _, r in lay]))) == sum(m for m, _, _ in lay)
    n = E.class_rows(128)["t3"] if dpad < 768 else E.FLOOD_END
    s = E.chain(q[:len(lay)], x[:n], dpad)
    for i, (m, where, rows) in enumerate(lay):
        assert rows.size == m and np.array_equal(rows, np.sort(rows))
        assert len({x[r].tobytes() for r in rows}) == 1
        sb = E.bits(s[i])
        assert len(set(sb[rows].tolist())) == 1, "copies with different score bits"
        others = np.delete(s[i], rows)
        assert s[i, rows[0]] > others.max(), f"cluster {i} is not its query's best"
        for k in (1, 32, 33, 112):
            es, er = E.expected_topk(s[i:i + 1], None, k)
            kk = min(k, m)
            assert np.array_equal(er[0, :kk], rows[:kk]) and (E.bits(es[0, :kk]) == sb[rows[0]]).all()
    sizes = {m for m, _, _ in lay}
    for k, cap in ((1, 64), (32, 64), (112, 128)):
        assert k + 1 in sizes and cap + 1 in sizes and any(m >= 3 * cap for m in sizes)
    # the placements, at the 3-tile row count of every RT (a unit of 384 rows = 4 / 2 / 1 whole chunks there)
    for rt, nq in ((32, 65), (64, 33), (128, 1)):
        p = E.plan(E.class_rows(rt)["t3"], nq, 1, dpad)
        chunk = p["RT"] * p["tiles_per_chunk"]
        assert p["tiles_per_chunk"] == 3 and E.UNIT % chunk == 0
        for m, where, rows in lay:
            chunks, tiles = np.unique(rows // chunk), np.unique(rows // rt)
            if where == "run" and m <= rt:
                assert tiles.size == 1, "a run no longer than a tile lies inside one tile"
            if where == "boundary":
                # (a run longer than a chunk of 96 rows cannot lie inside one: up to 65 copies do for every RT)
                assert tiles.size >= 2 and (m > 65 or chunks.size == 1), "a run across a tile boundary inside one chunk"
            if where == "spread" and m >= 33:
                assert chunks.size >= 3
                first = rows[rows // chunk == chunks[0]]
                assert first.size < 8 and (first // rt == (chunks[0] + 1) * p["tiles_per_chunk"] - 1).all(), "the lowest ids: few, in the LAST tile of their chunk"
                assert (np.bincount((rows // chunk - chunks[0]).astype(np.int64))[1:] > 0).sum() >= 2


@pytest.mark.parametrize("dim", list(E.DIMS))
@pytest.mark.parametrize("kind", ["rising", "falling"])
def test_monotone_corpora_are_monotone_on_the_chain_scores(kind, dim):
    dpad = E.DIMS[dim]
    x, q = E.corpus(kind, dim)
    n = min(E.rows_max(dpad), 40_000)
    qs = q[np.r_[0:8, 120:136]]
    s = E.chain(qs, x[:n], dpad)
    assert (s > 0).all()
    run = np.maximum.accumulate(s, axis=1)
    if kind == "rising":
        frac = (s[:, 1:] > run[:, :-1]).mean(axis=1)
        assert frac.min() >= 0.99, f"only {frac.min():.4f} of the rows are a running maximum"
    else:
        assert (s[:, 1:] > run[:, :-1]).sum() == 0 or (s[:, 1:] > run[:, :-1]).mean() < 1e-3
        assert (s[:, 112:] >= np.sort(s[:, :112], axis=1)[:, :1]).mean() < 0.01, "rows behind the first k still pass"


def test_zero_query_expects_the_first_rows_and_zero_bits():
    x, q = E.corpus("random", 100)
    assert not q[E.ZERO_QUERY].any()
    s = E.chain(q[E.ZERO_QUERY:E.ZERO_QUERY + 1], x[:5000], 192)
    assert (E.bits(s) == 0).all()
    es, er = E.expected_topk(-s, None, 33)                       # (-0.0 scores: normalised as the key does)
    assert (E.bits(es) == 0).all() and np.array_equal(er[0], np.arange(33))


def test_expected_topk_orders_pads_and_drops():
    s = np.array([[1.0, np.nan, 3.0, 3.0, -0.0, 0.0, 2.0]], np.float32)
    alive = np.array([1, 1, 1, 1, 1, 1, 0], bool)
    es, er = E.expected_topk(s, alive, 7)
    assert er[0].tolist() == [2, 3, 0, 4, 5, -1, -1]
    assert E.bits(es)[0].tolist() == E.bits(np.array([3, 3, 1, 0, 0, -np.inf, -np.inf], np.float32)).tolist()
    es, er = E.expected_topk(s, alive, 2)
    assert er[0].tolist() == [2, 3]
    ls, lr = E.expected_topk(s, alive, 7, qn2=np.array([2.5], np.float32))
    assert lr[0].tolist() == er[0].tolist() + [0, 4, 5, -1, -1] and ls[0].tolist() == [0.0, 0.0, 1.5, 2.5, 2.5, np.inf, np.inf]


def test_image_restatements():
    rng = np.random.default_rng(5)
    v = rng.standard_normal((9, 100)).astype(np.float32) * np.float32(3.0)
    s = E.cflat.wave_sumsq(E.pad(v, 192), 192)
    assert np.abs(s.astype(np.float64) - (v.astype(np.float64) ** 2).sum(1)).max() < 1e-4 * s.max()
    # one lane's chain and the butterfly, by hand, for a row longer than a wave
    row = E.pad(v[:1], 192)[0]
    lanes = np.zeros(64, np.float32)
    for c in range(192):
        lanes[c % 64] = np.float32(np.float64(row[c]) * np.float64(row[c]) + np.float64(lanes[c % 64]))      # (no midpoint here: checked below)
    for o in (32, 16, 8, 4, 2, 1):
        lanes = (lanes + lanes[np.arange(64) ^ o]).astype(np.float32)
    assert abs(float(lanes[0]) - float(s[0])) <= 2 * np.spacing(np.float32(s[0]))
    img = E.row_norm_image(v, 192)
    assert img.shape == (9, 192) and not img[:, 100:].any() and np.abs(np.linalg.norm(img.astype(np.float64), axis=1) - 1).max() < 1e-6
    assert not E.row_norm_image(np.zeros((1, 100), np.float32), 192).any()
    xi = E.l2_rows_image(v, 100, 192)
    assert np.array_equal(xi[:, :100], v) and np.array_equal(xi[:, 100], -E.cflat.wave_sumsq(E.pad(v, 192), 100)) and not xi[:, 101:].any()
    qi, qn2 = E.l2_queries_image(v, 100, 192)
    assert np.array_equal(qi[:, :100], 2 * v) and (qi[:, 100] == 1).all() and np.array_equal(qn2, -xi[:, 100])
    d = E.l2_merge(qn2, E.chain(qi, xi, 192))
    ref = ((v.astype(np.float64)[:, None, :] - v.astype(np.float64)[None, :, :]) ** 2).sum(2)
    assert np.abs(d - ref).max() < 1e-3 and (d >= 0).all()
