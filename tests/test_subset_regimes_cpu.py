"""The gathered exact scan's regimes, lists and reference, guarded without a GPU.

tests/subset_regimes.py restates rmu_subset_plan (with the SCfg table) and rmu_groups_plan (tpw, c_g, Pcap, the deal over the XCDs, the
null descriptors), builds the row lists and lists the cases; tests/test_subset_regimes_gpu.py holds `scan_subset_kernel` and
`scan_groups_kernel` to them.  Here:
  * every restated constant is read back out of scan_subset.hip / rmu_api.hip (those shared with the exact scan -- rmu_plan_chunks,
    block_map, ScanGeom's LDS terms, RMU_MAX_K -- through the table of tests/test_exact_regimes_cpu.py): a rework that moves one fails
    here, naming it, and the GPU cases have to follow;
  * the invariants of both planners hold over many shapes, and two small grouped plans equal tables worked by hand;
  * every list a case uses has the properties it is built for, proved from the restated plan alone: no position holds its own row id,
    some but not all copies of every flood cluster and never its lowest id, more than a full slot of the clusters sized for the slots,
    and the aimed cluster across a tile boundary of the list (not one of the corpus) and a chunk boundary of the plan;
  * the cases reach every (width, configuration, tile class), both block-map branches with one and two query tiles, every nq / k
    boundary from both sides, both group classes, a table with null descriptors and a Pcap-bound call;
  * the list reference equals E.expected_topk under the membership mask.
"""
import re

import numpy as np
import pytest

from tests import exact_regimes as E
from tests import subset_regimes as S
from tests import test_exact_regimes_cpu as XC

_STALE = "the gathered scan's planner moved: update tests/subset_regimes.py and its GPU cases (tests/test_subset_regimes_gpu.py)"


def _subset():
    return XC._read("ragmeup_amd/csrc/scan_subset.hip")


_IDS_LEN = r"int64_t rmu_subset_ids_len\(int64_t n_sub\) \{ return \(n_sub \+ (\d+)\) / (\d+) \* (\d+) \+ (\d+); \}"
_TPW = r"const int64_t tpw = work > (\d+) \? \(work \+ (\d+)\) / (\d+) : 1;"
_PCAP = r"int pcap = \(int\)\(\(1ll << (\d+)\) / slots\); pcap = pcap > (\d+) \? (\d+) : \(pcap < (\d+) \? (\d+) : pcap\);"
_W4K0 = r"template <int D> using S_w4_k0 = SCfg<D, (\d+), D == (\d+) \? (\d+) : (\d+), (\d+), (\d+)>;"


def _row(name):
    return r"template <int D> using %s = SCfg<D, (\d+), (\d+), (\d+), (\d+)>;" % name


# name -> (where, pattern, group, restated value)
SOURCE_CONSTANTS = {
    "rmu_subset_plan: kv = k <= 32": (_subset, r"p->kv = p->k <= (\d+) \? 0 : 1;", 1, S.K_SPLIT),
    "rmu_subset_plan: wq = 1 for nq <= 32": (_subset, r"p->wq = \(p->nq <= (\d+) && p->kv == 0\) \? 1 : 4;", 1, S.NQ_W1),
    "SCfg: RING": (_subset, r"struct SCfg : ScanGeom<D_, WQ_, CKF_, (\d+), CAP_, NCHECK_> \{ using G = ScanGeom<D_, WQ_, CKF_, (\d+), CAP_, NCHECK_>;", 1, S.S_RING),
    "SCfg: RING (G)": (_subset, r"struct SCfg : ScanGeom<D_, WQ_, CKF_, (\d+), CAP_, NCHECK_> \{ using G = ScanGeom<D_, WQ_, CKF_, (\d+), CAP_, NCHECK_>;", 2, S.S_RING),
    "SCfg: the landing zone of the row ids 4 * 512": (_subset, r"LDS_BYTES = IDS_OFF \+ (\d+) \* (\d+);", (1, 2), S.IDS_BYTES),
    "S_w4_k0: WQ": (_subset, _W4K0, 1, 4),
    "S_w4_k0: the narrow width": (_subset, _W4K0, 2, 192),
    "S_w4_k0: CKF at 192": (_subset, _W4K0, 3, S.S_W4_K0_CKF_192),
    "S_w4_k0: CKF": (_subset, _W4K0, 4, S.S_CFG[(4, 0)][0]),
    "S_w4_k0: CAP": (_subset, _W4K0, 5, S.S_CFG[(4, 0)][1]),
    "S_w4_k0: NCHECK": (_subset, _W4K0, 6, S.S_CFG[(4, 0)][2]),
    "rmu_subset_ids_len: + 127": (_subset, _IDS_LEN, 1, S.IDS_ROUND - 1),
    "rmu_subset_ids_len: / 128": (_subset, _IDS_LEN, 2, S.IDS_ROUND),
    "rmu_subset_ids_len: * 128": (_subset, _IDS_LEN, 3, S.IDS_ROUND),
    "rmu_subset_ids_len: + 128": (_subset, _IDS_LEN, 4, S.IDS_ROUND),
    "rmu_groups_plan: kv = k <= 32": (_subset, r"const int kv = k <= (\d+) \? 0 : 1; struct Grp", 1, S.K_SPLIT),
    "rmu_groups_plan: class 0 for <= 32 queries": (_subset, r"g\.cls = \(g\.cnt <= (\d+) && kv == 0\) \? 0 : 1;", 1, S.NQ_W1),
    "rmu_groups_plan: tpw, work > 256": (_subset, _TPW, 1, S.WORK_WAVE),
    "rmu_groups_plan: tpw, + 255": (_subset, _TPW, 2, S.WORK_WAVE - 1),
    "rmu_groups_plan: tpw, / 256": (_subset, _TPW, 3, S.WORK_WAVE),
    "rmu_groups_plan: Pcap, 2^25 slots": (_subset, _PCAP, 1, S.PCAP_SLOTS.bit_length() - 1),
    "rmu_groups_plan: Pcap, above 1024": (_subset, _PCAP, 2, S.PCAP_MAX),
    "rmu_groups_plan: Pcap, 1024": (_subset, _PCAP, 3, S.PCAP_MAX),
    "rmu_groups_plan: Pcap, below 4": (_subset, _PCAP, 4, S.PCAP_MIN),
    "rmu_groups_plan: Pcap, 4": (_subset, _PCAP, 5, S.PCAP_MIN),
    "rmu_groups_plan: 8 XCDs (lists)": (_subset, r"std::vector<GroupDesc> per_xcd\[2\]\[(\d+)\];", 1, S.XCDS),
    "rmu_groups_plan: 8 XCDs (deal)": (_subset, r"int xcd = 0; for \(int x = 1; x < (\d+); \+\+x\) if \(per_xcd\[g\.cls\]\[x\]\.size\(\) < per_xcd\[g\.cls\]\[xcd\]\.size\(\)\) xcd = x;", 1, S.XCDS),
    "rmu_groups_plan: 8 XCDs (table length)": (_subset, r"out->tab\[cls\]\.assign\(longest \* (\d+), GroupDesc\{0u, 0u, 0u, 0u, 0u, 0u, \{0u, 0u\}\}\);", 1, S.XCDS),
    "rmu_groups_plan: 8 XCDs (table order)": (_subset, r"out->tab\[cls\]\[m \* (\d+) \+ x\] = per_xcd\[cls\]\[x\]\[m\];", 1, S.XCDS),
    "rmu_index_search_groups: at most 8192 queries": (XC._api, r"static const int64_t kMaxQueriesPerLaunch = (\d+);", 1, S.MAX_QUERIES),
}
for _name, _key in (("S_w1_k0", (1, 0)), ("S_w4_k1", (4, 1))):
    SOURCE_CONSTANTS[f"{_name}: WQ"] = (_subset, _row(_name), 1, _key[0])
    for _g, _what in enumerate(("CKF", "CAP", "NCHECK")):
        SOURCE_CONSTANTS[f"{_name}: {_what}"] = (_subset, _row(_name), _g + 2, S.S_CFG[_key][_g])
# what the gathered planners share with the exact scan, read back where the exact pin reads it
SHARED = [n for n in XC.SOURCE_CONSTANTS if n.startswith(("rmu_plan_chunks", "block_map", "ScanGeom", "RMU_MAX_K"))]

SOURCE_SHAPES = {
    "the widths: 192, 384, 768": r"int rmu_subset_plan\(SubsetLaunch\* p\) \{.*?if \(p->dpad != 192 && p->dpad != 384 && p->dpad != 768\) return RMU_E_INVALID;",
    "rows per tile: 32 * (4 / wq)": r"const int rt = 32 \* \(4 / p->wq\); p->nqt = \(p->nq \+ 32 \* p->wq - 1\) / \(32 \* p->wq\);",
    "chunks from the planner": r"rmu_plan_chunks\(p->nqt, \(p->n_sub \+ rt - 1\) / rt, &p->s_chunks, &p->tiles_per_chunk\);",
    "grid and parts": r"p->grid = p->s_chunks \* p->nqt; p->parts = p->s_chunks \* \(4 / p->wq\);",
    "with_cfg": r"switch \(wq \* 2 \+ kv\) \{ case 2: return f\(S_w1_k0<D>\{\}\); case 8: return f\(S_w4_k0<D>\{\}\); case 9: return f\(S_w4_k1<D>\{\}\); default: return RMU_E_INVALID; \}",
    "SCfg: the ids follow ScanGeom's tail": r"IDS_OFF = G::TAIL_OFF;",
    "block map of the subset kernel": r"block_map\(a\.s_chunks, a\.nqt, s_idx, qt\);.*subset_scan<C>\(sa, a\.ids, t0, ntiles, qt \* C::WQ \* 32, a\.nq, s_idx \* C::RP\);",
    "groups: a group is a run of q_list": r"while \(q1 < nq && q_list\[q1\] == q_list\[q0\]\) \+\+q1;",
    "groups: an empty list has no group": r"if \(len > 0\) \{",
    "groups: geometry of a group": r"const int wq = g\.cls \? 4 : 1, rt = 32 \* \(4 / wq\); g\.nqt = \(g\.cnt \+ 32 \* wq - 1\) / \(32 \* wq\); g\.tiles = \(len \+ rt - 1\) / rt;",
    "groups: ids end to end": r"g\.ids_off = \(u32\)out->ids_total;.*out->ids_total \+= rmu_subset_ids_len\(len\);",
    "groups: work": r"work \+= g\.tiles \* g\.nqt;",
    "groups: pcap from nq * k": r"const int64_t slots = \(int64_t\)nq \* k;",
    "groups: c_g, tpc and the second rounding": r"int64_t c = \(g\.tiles \+ tpw - 1\) / tpw; if \(c > pcap / rp\) c = pcap / rp; const int64_t tpc = \(g\.tiles \+ c - 1\) / c; "
                                                r"c = \(g\.tiles \+ tpc - 1\) / tpc;",
    "groups: parts": r"if \(\(int\)c \* rp > out->parts\) out->parts = \(int\)c \* rp;",
    "groups: descriptors of a chunk": r"const int64_t t0 = ch \* tpc, t1 = t0 \+ tpc < g\.tiles \? t0 \+ tpc : g\.tiles; for \(int qt = 0; qt < g\.nqt; \+\+qt\) "
                                      r"per_xcd\[g\.cls\]\[xcd\]\.push_back\(GroupDesc\{g\.ids_off, \(u32\)t0, \(u32\)\(t1 - t0\), \(u32\)\(g\.q0 \+ qt \* 32 \* wq\), "
                                      r"\(u32\)\(g\.q0 \+ g\.cnt\), \(u32\)\(ch \* rp\), \{0u, 0u\}\}\);",
    "groups: LDS bytes per class": r"with_cfg<decltype\(d\)::value>\(cls \? 4 : 1, cls \? kv : 0,",
    "keys carry list positions": r"const u32 pos0 = \(u32\)\(\(t0 \+ tl\) \* C::RT\) \+ \(u32\)\(32 \* rp \+ 4 \* h\);",
    "the filter is strict": r"pmask \|= \(acc\[r\] > thr\) \? \(1u << r\) : 0u;",
    "the key normalises -0.0": r"rmu_make_key\(acc\[r\] \+ 0\.0f, pos0 \+ \(u32\)\(\(r & 3\) \+ 8 \* \(r >> 2\)\)\);",
    "an absent id is outside [0, n)": r"if \(r >= 0 && r < n_rows\) v = \(u32\)r;",
}
API_SHAPES = {
    "one launch noted per subset search": r"rc = rmu_subset_launch\(&L, s\);.*?t\.note_geometry\(L, 1\); parts = L\.parts;",
    "one launch noted per class": r"for \(int cls = 0; cls < 2; \+\+cls\) \{ if \(P\.tab\[cls\]\.empty\(\)\) continue;.*?L\.grid = \(int\)P\.tab\[cls\]\.size\(\); L\.lds_bytes = P\.lds_bytes\[cls\];"
                                  r".*?t\.note_geometry\(L, 1\);",
    "note_geometry overwrites grid and LDS bytes and adds launches": r"void note_geometry\(const Launch& L, int launches\) \{ grid = L\.grid; block = 256; lds = L\.lds_bytes; passes \+= launches; \}",
}


@pytest.mark.parametrize("name", list(SOURCE_CONSTANTS))
def test_restated_constant_equals_the_source(name):
    where, pat, group, restated = SOURCE_CONSTANTS[name]
    m = re.search(pat, where())
    assert m, f"{name}: not found in the source any more -- {_STALE}"
    assert XC._value(m, group) == restated, f"{name}: the source says {XC._value(m, group)}, tests/subset_regimes.py says {restated} -- {_STALE}"


@pytest.mark.parametrize("name", SHARED)
def test_constant_shared_with_the_exact_scan_equals_the_source(name):
    XC.test_restated_constant_equals_the_source(name)


def test_the_shared_constants_are_all_there():
    assert len(SHARED) == 12 and {"RMU_MAX_K", "block_map: s_chunks & 7", "ScanGeom: trash 256 * 8"} <= set(SHARED)


@pytest.mark.parametrize("name", list(SOURCE_SHAPES))
def test_restated_structure_is_in_the_source(name):
    assert re.search(SOURCE_SHAPES[name], _subset()), f"{name}: not found in scan_subset.hip any more -- {_STALE}"


@pytest.mark.parametrize("name", list(API_SHAPES))
def test_what_last_geometry_reports_is_in_the_source(name):
    assert re.search(API_SHAPES[name], XC._api()), f"{name}: not found in rmu_api.hip any more -- {_STALE}"


def test_lds_bytes_against_the_static_limit_and_the_header_s_figures():
    for (wq, kv), (ckf, cap, ncheck) in S.S_CFG.items():
        for dpad in E.WIDTHS:
            p = S.subset_plan(10_000, 32 if wq == 1 else 128, 32 if kv == 0 else 33, dpad)
            ckf_d = S.S_W4_K0_CKF_192 if (wq, kv, dpad) == (4, 0, 192) else ckf
            assert (p["wq"], p["kv"]) == (wq, kv) and p["lds_bytes"] <= 160 * 1024 and dpad % ckf_d == 0
            assert dpad // ckf_d >= 3                                      # SCfg's static_assert: NCH >= 3
            assert (E.K_SPLIT if kv == 0 else E.MAX_K) + p["A"] <= cap     # k + A <= CAP
    ring = lambda wq, kv, dpad: S.lds_bytes(wq, kv, dpad) - 4 * 32 * S.S_CFG[(wq, kv)][1] * 8 - E.LDS_CNT - E.LDS_THR - E.LDS_TRASH - S.IDS_BYTES
    # the comments of the geometry table: 72 KiB ring; 36 KiB (12 KiB at 192); 12 KiB
    assert [ring(1, 0, 384), ring(4, 0, 384), ring(4, 0, 192), ring(4, 1, 768)] == [72 * 1024, 36 * 1024, 12 * 1024, 12 * 1024]
    assert S.ids_len(0) == 128 and S.ids_len(1) == 256 and S.ids_len(128) == 256 and S.ids_len(129) == 384


# ---- planner invariants ---------------------------------------------------------------------------------------------------------------
def test_subset_plan_follows_the_boundaries_and_partitions_the_tiles():
    seen = set()
    for nq in (1, 31, 32, 33, 64, 65, 128, 129, 256, 257, 300, 8192):
        for k in (1, 32, 33, 112):
            for n_sub in (0, 1, 31, 32, 33, 127, 128, 129, 4096, 8192, 8225, 32768, 32897, 65665, 70_001, 139_999):
                p = S.subset_plan(n_sub, nq, k, 384)
                assert p["config"] == ("S_w1_k0" if (nq <= 32 and k <= 32) else "S_w4_k0" if k <= 32 else "S_w4_k1")
                assert p["RT"] == (128 if p["wq"] == 1 else 32) and p["nqt"] * 32 * p["wq"] >= nq > (p["nqt"] - 1) * 32 * p["wq"]
                assert p["grid"] == p["s_chunks"] * p["nqt"] and p["parts"] == p["s_chunks"] * 4 // p["wq"] <= 1024
                if n_sub:
                    assert (p["s_chunks"] - 1) * p["tiles_per_chunk"] < p["tiles_total"] <= p["s_chunks"] * p["tiles_per_chunk"]
                    assert 0 < p["tiles_last_chunk"] <= p["tiles_per_chunk"]
                assert p["ids_len"] >= p["tiles_total"] * p["RT"] + 64       # RT = 32: lanes 32..63 read the ids of the tile behind the last
                seen.add(p["config"])
    assert seen == set(S.CONFIGS)
    assert S.subset_plan(100, 1, 33, 384)["config"] == "S_w4_k1" and S.subset_plan(100, 32, 33, 384)["config"] == "S_w4_k1"    # no promoted w2


def test_the_list_lengths_of_each_tile_class():
    assert [S.class_lengths(128)[c] for c in ("t1_xcd", "t2", "t3")] == [256 * 128, 32_897, 65_665]
    assert [S.class_lengths(32)[c] for c in ("t1_xcd", "t2", "t3", "t4")] == [256 * 32, 8_225, 16_417, 24_609]
    for rt, nq, k, nqt in ((128, 1, 1, 1), (32, 33, 1, 1), (32, 128, 112, 1), (32, 129, 32, 2), (32, 256, 33, 2)):
        ln = S.class_lengths(rt, nqt)
        for name, tpc in (("sub", 1), ("one", 1), ("t1_xcd", 1), ("t2", 2), ("t3", 3), ("t3_full", 3)) + ((("t4", 4),) if rt == 32 else ()):
            p = S.subset_plan(ln[name], nq, k, 384)
            assert (p["RT"], p["nqt"], p["tiles_per_chunk"]) == (rt, nqt, tpc), (rt, nqt, name, p)
            if name in ("t2", "t3", "t4"):                       # the smallest such length: two tiles fewer is one class less
                assert ln[name] % rt == 1 and S.subset_plan(ln[name] - 1 - rt, nq, k, 384)["tiles_per_chunk"] == tpc - 1
        assert S.subset_plan(ln["t1_xcd"], nq, k, 384)["xcd_branch"] and ln["t1_xcd"] % rt == 0
        assert ln["t3_full"] % rt == rt - 1 and ln["sub"] < rt and ln["one"] == rt
        assert S.subset_plan(ln["sub"], nq, k, 384)["grid"] == nqt and S.subset_plan(ln["one"], nq, k, 384)["tiles_total"] == 1
    assert E.plan_chunks(1, 1 << 20)[0] == 256 and E.plan_chunks(2, 1 << 20)[0] == 128


def test_two_grouped_plans_worked_by_hand():
    # one query, 300 rows, k = 10: class 0, 3 tiles of 128, W = 3, tpw = 1: three chunks of one tile on XCDs 0, 1, 2, four row parts each
    p = S.groups_plan(384, 10, [300], [0])
    assert (p["work"], p["tpw"], p["pcap"], p["parts"], p["ids_total"], p["launches"], p["grid"]) == (3, 1, 1024, 12, 512, 1, 8)
    assert p["tab"][0] == [(0, 0, 1, 0, 1, 0), (0, 1, 1, 0, 1, 4), (0, 2, 1, 0, 1, 8)] + [S.NULL_DESC] * 5 and p["tab"][1] == []
    assert p["last_lds_bytes"] == S.lds_bytes(1, 0, 384)
    # 2 queries on 40 rows, 3 on an empty list, 40 on 70 rows, k = 33: class 1 both; lists of 2 and 3 tiles of 32; W = 2 + 3 * 1 = 5
    p = S.groups_plan(192, 33, [40, 0, 999, 70], [0, 0, 1, 1, 1] + [3] * 40)
    assert (p["work"], p["tpw"], p["parts"], p["ids_total"], p["launches"], p["grid"]) == (5, 1, 3, 256 + 256, 1, 8)
    assert p["q_off"] == [0, 0, 0, 0, 0] + [256] * 40
    assert p["tab"][1] == [(0, 0, 1, 0, 2, 0), (0, 1, 1, 0, 2, 1), (256, 0, 1, 5, 45, 0), (256, 1, 1, 5, 45, 1), (256, 2, 1, 5, 45, 2)] + [S.NULL_DESC] * 3
    assert p["last_lds_bytes"] == S.lds_bytes(4, 1, 192) and p["tab"][0] == []
    # the Pcap example of the planner's comment, by hand: nq = 8192, k = 112 -> 2^25 / 917504 = 36
    assert S.PCAP_SLOTS // (8192 * 112) == 36


def test_grouped_plans_cover_every_tile_once_within_their_bounds():
    rng = np.random.default_rng(7)
    for trial in range(60):
        k = int(rng.choice([1, 32, 33, 112]))
        n_lists = int(rng.integers(1, 9))
        lens = [int(v) for v in rng.choice([0, 1, 31, 32, 33, 127, 128, 129, 1000, 5000, 20_000, 70_000], n_lists)]
        counts = [int(v) for v in rng.choice([0, 1, 31, 32, 33, 128, 129, 300, 2000], n_lists)]
        q_list = [li for li, c in enumerate(counts) for _ in range(c)] or [0]
        p = S.groups_plan(384, k, lens, q_list)
        nq = len(q_list)
        assert p["parts"] * nq * k * 8 <= 256 << 20 or p["parts"] <= 4
        assert p["work"] == sum(g["tiles"] * g["nqt"] for g in p["groups"]) and p["ids_total"] == sum(S.ids_len(g["len"]) for g in p["groups"])
        if not any(g["pcap_bound"] for g in p["groups"]):
            assert sum(g["c"] * g["nqt"] for g in p["groups"]) <= 256 + sum(g["nqt"] for g in p["groups"])
        for cls in (0, 1):
            real = [d for d in p["tab"][cls] if d != S.NULL_DESC]
            assert len(p["tab"][cls]) % S.XCDS == 0 and len(real) == sum(g["c"] * g["nqt"] for g in p["groups"] if g["cls"] == cls)
            if real:
                per = [sum(1 for d in p["tab"][cls][x::S.XCDS] if d != S.NULL_DESC) for x in range(S.XCDS)]
                assert max(per) * S.XCDS == len(p["tab"][cls]) and max(per) - min(per) <= max(g["nqt"] for g in p["groups"] if g["cls"] == cls)
                for x in range(S.XCDS):                              # the nulls of an XCD follow its descriptors
                    col = [d != S.NULL_DESC for d in p["tab"][cls][x::S.XCDS]]
                    assert col == sorted(col, reverse=True)
        for g in p["groups"]:
            assert g["ids_off"] % S.IDS_ROUND == 0 and g["c"] * g["RP"] <= max(p["pcap"], g["RP"]) and g["c"] * g["RP"] <= p["parts"]
            assert g["tpc"] <= p["tpw"] or g["pcap_bound"]
            mine = [(x, d) for x in range(S.XCDS) for d in p["tab"][g["cls"]][x::S.XCDS] if d != S.NULL_DESC and d[0] == g["ids_off"]]
            for qt in range(g["nqt"]):
                tiles = sorted(t for _, d in mine if d[3] == g["q0"] + qt * 32 * g["wq"] for t in range(d[1], d[1] + d[2]))
                assert tiles == list(range(g["tiles"])), "a tile is scanned twice or never"
            assert all(d[4] == g["q0"] + g["cnt"] and d[5] == (d[1] // g["tpc"]) * g["RP"] and 0 < d[2] <= g["tpc"] for _, d in mine)
            for ch in range(g["c"]):                                 # the query tiles of one chunk share an XCD
                assert len({x for x, d in mine if d[1] == ch * g["tpc"]}) == 1


# ---- the lists ----------------------------------------------------------------------------------------------------------------------------
def _lists_in_use():
    """(list length, span, chunk) -> the plans (configuration, RT, tiles per chunk, CAP) it runs under"""
    out = {}
    for c in S.CASES:
        p = c.plan
        out.setdefault((c.length, c.n, p["RT"] * p["tiles_per_chunk"]), set()).add((p["config"], p["RT"], p["tiles_per_chunk"], p["CAP"]))
    return out


def test_every_list_differs_from_its_positions_and_lies_in_its_index():
    for (length, span, chunk), plans in _lists_in_use().items():
        rows = S.make_list(length, span, chunk)
        assert rows.dtype == np.int64 and rows.size == length and (np.diff(rows) > 0).all() and not rows.flags.writeable
        assert rows[0] >= S.SKIP and rows[-1] < span and (rows > np.arange(length)).all(), "a position holds its own row id"
        assert np.array_equal(rows, S.make_list(length, span, chunk))
    for c in S.CASES:
        assert c.n <= S.N_ROWS[c.dpad] and c.length < S.N_ROWS[c.dpad]
    assert S.N_ROWS[192] == S.N_ROWS[384] == E.rows_max(384) and E.rows_max(768) < S.class_lengths(128)["t3_full"] < S.N_ROWS[768] <= 72_000


def test_consecutive_tiles_of_a_list_gather_from_far_apart_rows():
    """an id taken one tile late returns other rows -- and rows that a contiguous list of the same start would not hold either"""
    for (length, span, chunk), plans in _lists_in_use().items():
        rows = S.make_list(length, span, chunk)
        for _, rt, _, _ in plans:
            if length >= S.FLOOD_MIN:
                filler = rows[~np.isin(rows, np.concatenate([r for _, _, r in E.flood_layout()]))]
                assert (np.diff(filler) > 1).mean() > 0.03, "the list is nearly contiguous"
                assert (rows[rt:] - rows[:-rt] > rt).mean() > 0.9, "a tile later is not farther than a tile of the corpus"


def test_flood_lists_hold_some_of_every_cluster_never_its_lowest_id_and_a_full_slot_across_the_boundaries():
    lay = E.flood_layout()
    assert lay[S.AIM][0] == 384 and lay[S.AIM][1] == "run"
    big = {(length, span, chunk): plans for (length, span, chunk), plans in _lists_in_use().items() if length >= S.FLOOD_MIN}
    small = {key: plans for key, plans in _lists_in_use().items() if key[0] < S.FLOOD_MIN}
    assert len(big) >= 12 and {key[0] for key in small} == {20, 32, 128}
    for (length, span, chunk), plans in big.items():
        rows = S.make_list(length, span, chunk)
        for m, where, cl in lay:
            here = np.isin(cl, rows)
            assert 0 < here.sum() < m and not here[0], f"cluster of {m} ({where}): all, none or the lowest id in the list"
            for cap, sizes in ((128, (384,)), (64, (384, 192))):            # (a cluster of CAP + 1 cannot lose its lowest id and still fill a slot)
                if m in sizes:
                    assert here.sum() >= cap + 1
            for k in (1, 32, 112):
                if m == k + 1:
                    assert here.sum() <= k, "the list holds k + 1 copies of a k + 1 cluster: it should have lost at least the lowest"
        pos = np.nonzero(np.isin(rows, lay[S.AIM][2]))[0]
        assert pos.size == S.held_copies(lay[S.AIM][2]).size == 328 and (np.diff(pos) == 1).all(), "the aimed cluster is one run of list positions"
        assert pos[0] % chunk == (chunk - S.BEFORE) % chunk
        for config, rt, tpc, cap in plans:
            assert chunk == rt * tpc
            inside = set(pos.tolist())
            chunk_b = [b for b in range(chunk, length, chunk) if b - 1 in inside and b in inside]
            tile_b = [b for b in range(rt, length, rt) if b - 1 in inside and b in inside and (tpc == 1 or b % chunk)]
            assert chunk_b and tile_b, f"L={length} {config}: the copies do not cross a chunk boundary and a tile boundary of the list"
            assert any(rows[b] % rt for b in tile_b), "the tile boundary of the list is one of the corpus too"
            sides = [(int(((pos >= b - chunk) & (pos < b)).sum()), int(((pos >= b) & (pos < b + chunk)).sum())) for b in chunk_b]
            before, after = max(sides, key=min)                  # the copies the two workgroups of the best-placed chunk boundary scan
            assert before >= min(chunk, S.BEFORE) and after >= min(chunk, pos.size - S.BEFORE)
            if rt == 128:                                        # S_w1_k0: more than CAP copies on either side of the boundary
                assert before > cap and after > cap
            assert pos.size >= cap + 1 and pos.size > E.MAX_K
    for (length, span, chunk), plans in small.items():           # up to one tile: two copies of a few clusters, never the lowest id
        rows = S.make_list(length, span, chunk)
        n_held = [int(np.isin(cl, rows).sum()) for _, _, cl in lay]
        assert sum(1 for v in n_held if v == 2) >= 4 and not any(np.isin(cl[0], rows) for _, _, cl in lay)


# ---- coverage of the cases --------------------------------------------------------------------------------------------------------------
def _grid():
    return [c for c in S.CASES if c.corpus == "random" and c.metric == "ip"]


def test_cases_reach_every_width_configuration_and_tile_class():
    seen = {(c.dpad, c.plan["config"], c.plan["tile_class"]) for c in _grid() if c.plan["nqt"] == 1}
    for dpad in E.WIDTHS:
        for config in S.CONFIGS:
            for t in (1, 2, 3) + ((4,) if config != "S_w1_k0" else ()):
                assert (dpad, config, t) in seen, f"{config} at dpad {dpad} never runs with {t} tiles per workgroup"
    assert {c.dim for c in S.CASES if c.metric != "l2"} == set(E.DIMS) and {c.dim for c in S.CASES if c.metric == "l2"} == set(E.L2_DIMS)
    assert {c.dim for c in _grid()} == set(E.DIMS)
    for dpad in E.WIDTHS:
        for config in S.CONFIGS:
            some = [c for c in _grid() if c.dpad == dpad and c.plan["config"] == config]
            rt = some[0].plan["RT"]
            assert any(c.plan["tiles_per_chunk"] == 3 and c.length % rt == rt - 1 for c in some), "no 3-tile length with L = RT - 1 mod RT"
            assert any(c.length < rt for c in some) and any(c.length == rt for c in some)
            assert any(c.plan["tiles_last_chunk"] < c.plan["tiles_per_chunk"] for c in some)


def test_cases_reach_both_block_map_branches_with_one_and_two_query_tiles():
    for dpad in E.WIDTHS:
        seen = {(c.plan["config"], c.plan["nqt"], c.plan["xcd_branch"]) for c in _grid() if c.dpad == dpad}
        for config in S.CONFIGS:
            assert {(config, 1, True), (config, 1, False)} <= seen
        for config in ("S_w4_k0", "S_w4_k1"):
            assert {(config, 2, True), (config, 2, False)} <= seen
            assert {c.plan["tiles_per_chunk"] for c in _grid() if c.dpad == dpad and c.plan["config"] == config and c.plan["nqt"] == 2} == {1, 2, 3}
        assert {(c.nq, c.k) for c in _grid() if c.dpad == dpad and c.plan["nqt"] == 2} == {(129, 32), (129, 112), (256, 33)}


def test_cases_reach_every_boundary_from_both_sides():
    for dpad in E.WIDTHS:
        shapes = {(c.nq, c.k): c.plan["config"] for c in _grid() if c.dpad == dpad}
        assert shapes[(32, 32)] == "S_w1_k0" and shapes[(33, 32)] == "S_w4_k0"                        # nq 32 | 33 at k <= 32
        assert shapes[(1, 32)] == "S_w1_k0" and shapes[(1, 33)] == "S_w4_k1" and shapes[(32, 33)] == "S_w4_k1"     # k 32 | 33 at nq <= 32
        assert shapes[(128, 32)] == shapes[(129, 32)] == "S_w4_k0" and shapes[(128, 112)] == shapes[(129, 112)] == "S_w4_k1"      # nq 128 | 129
        for config in S.CONFIGS:
            ks = {k for (nq, k), cfg in shapes.items() if cfg == config}
            assert ks >= ({1, 32} if config != "S_w4_k1" else {33, 112}), (config, ks)
    mono = [c for c in S.CASES if c.corpus in ("rising", "falling")]
    for kind in ("rising", "falling"):
        for dim in E.DIMS:
            mine = [c for c in mono if c.corpus == kind and c.dim == dim]
            assert {c.k for c in mine} == {1, 32, 33, 112}
            assert {(c.plan["config"], c.plan["tiles_per_chunk"]) for c in mine} == {("S_w1_k0", 3), ("S_w4_k0", 4), ("S_w4_k1", 4)}
    for metric, dims in (("cosine", (100, 384, 768)), ("l2", (100, 383, 767))):
        for dim in dims:
            mine = [c for c in S.CASES if c.metric == metric and c.dim == dim]
            assert {c.plan["config"] for c in mine} == set(S.CONFIGS) and all(c.plan["tiles_per_chunk"] >= 2 and c.corpus == "scaled" for c in mine)


def test_grouped_calls_reach_both_classes_three_tiles_null_descriptors_and_pcap():
    calls = {c.name: c for c in S.group_calls(384)}
    for name, cls, kv in (("one_group_w1_tpw3", 0, 0), ("one_group_w4_k0_tpw3", 1, 0), ("one_group_w4_k1_tpw3", 1, 1)):
        p = calls[name].plan
        g, = p["groups"]
        assert (p["work"], p["tpw"], g["cls"], g["tpc"], p["classes"], p["launches"]) == (514, 3, cls, 3, [cls], 1) and (calls[name].k > 32) == bool(kv)
        assert max(d[2] for d in p["tab"][cls]) == 3 and p["grid"] == len(p["tab"][cls]) and p["last_lds_bytes"] == S.lds_bytes(4 if cls else 1, kv, 384)
    assert len(calls["one_group_w1_tpw3"].lists[0]) >= 65_665
    m = calls["mixed"]
    p = m.plan
    assert p["tpw"] >= 2 and p["classes"] == [0, 1] and p["launches"] == 2 and p["grid"] == len(p["tab"][1])
    assert sorted(len(q) for _, q in m.groups) == [1, 5, 31, 32, 33, 128, 129]
    assert sum(1 for g in p["groups"] if g["q0"] % 32) >= 4, "the group boundaries should fall inside a 32-lane query fragment"
    assert all(any(d[4] < d[3] + 32 * g["wq"] * 1 and d[4] % 32 for d in p["tab"][g["cls"]] if d[0] == g["ids_off"]) for g in p["groups"] if g["cnt"] % 32)
    assert p["nulls"][0] > 0 and p["nulls"][1] > 0
    for cls in (0, 1):
        assert sum(g["c"] for g in p["groups"] if g["cls"] == cls) % 8, "the chunk count of a class should not be a multiple of 8"
        assert max(d[2] for d in p["tab"][cls]) >= 2
    lens = [len(v) for v in m.lists]
    used = [li for li, _ in m.groups]
    assert lens[2] == 0 and 2 in used and used.index(2) not in (0, len(used) - 1), "an empty list between two used ones"
    assert 4 not in used and lens[4] > 0, "a list nobody uses"
    assert np.isin(m.lists[7], m.lists[6]).all() and 6 in used and 7 in used, "two overlapping lists"
    assert len(set(lens)) == len(lens)
    pc = calls["pcap"].plan
    small, bound = pc["groups"]
    assert len(calls["pcap"].q_list) == S.MAX_QUERIES and calls["pcap"].k == 112 and pc["pcap"] == 36
    assert (small["cnt"], small["tiles"] * small["nqt"], bound["cnt"], bound["tiles"], bound["nqt"]) == (8063, 63, 129, 200, 2)
    assert (pc["work"], pc["tpw"]) == (463, 2) and bound["pcap_bound"] and not small["pcap_bound"]
    assert -(-bound["tiles"] // (pc["pcap"] // bound["RP"])) == bound["tpc"] == 6 > pc["tpw"] and bound["c"] == 34 and pc["parts"] == 34
    assert pc["parts"] * S.MAX_QUERIES * 112 * 8 <= 256 << 20
    for name in ("flood", "flood_k112"):
        c = calls[name]
        grid_lists = {key[0] for key in _lists_in_use()}
        assert all(len(v) in grid_lists and len(v) >= S.FLOOD_MIN for v in c.lists) and all(set(range(24)) <= set(q.tolist()) for _, q in c.groups)
    assert calls["flood"].plan["classes"] == [0, 1] and calls["flood_k112"].plan["classes"] == [1]
    assert max(g["tpc"] for g in calls["flood_k112"].plan["groups"]) >= 4          # 128 positions of one cluster in one workgroup: a CAP 128 slot fills
    for c in calls.values():
        assert c.n <= S.N_ROWS[384] and all((np.diff(v) > 0).all() for v in c.lists if len(v) > 1)


# ---- the reference ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["ip", "l2"])
def test_the_list_reference_is_expected_topk_under_the_membership_mask(metric):
    from types import SimpleNamespace
    n = E.FLOOD_END
    ref = S.Reference(100, "scaled", metric, [SimpleNamespace(nq=32, n=n), SimpleNamespace(nq=S.NQ_MAX, n=n)])
    rows = S.make_list(8225, n, 64)
    qn2 = None if ref.qn2 is None else ref.qn2[:32]
    member = np.zeros(n, bool)
    member[rows] = True
    for k in (1, 33, 112):
        assert E.mismatch(*ref.expected(rows, 32, k), *E.expected_topk(ref.scores[32], member, k, qn2)) == ""
    if metric == "ip":       # an answer that ignores membership is wrong at rank 0 for every query aimed at a cluster (`random`: the cluster is its best)
        rnd = S.Reference(100, "random", "ip", [SimpleNamespace(nq=32, n=n)])
        assert (rnd.expected(rows, 24, 1)[1][:, 0] != E.expected_topk(rnd.scores[32][:24], None, 1)[1][:, 0]).all()
    # removed rows, absent ids, row_base, chosen queries, fewer live rows than k
    alive = np.ones(rows.size, bool)
    alive[::3] = False
    gone = member.copy()
    gone[rows[::3]] = False
    assert E.mismatch(*ref.expected(rows, 32, 33, alive=alive), *E.expected_topk(ref.scores[32], gone, 33, qn2)) == ""
    holed = np.array(rows)
    holed[::3] = [(n + i, (1 << 32) + i, -1 - i)[i % 3] for i in range(holed[::3].size)]
    assert E.mismatch(*ref.expected(holed, 32, 33), *E.expected_topk(ref.scores[32], gone, 33, qn2)) == ""
    s0, r0 = ref.expected(rows, 32, 33)
    s1, r1 = ref.expected(rows, 32, 33, row_base=1000)
    assert np.array_equal(E.bits(s0), E.bits(s1)) and np.array_equal(r1, r0 + 1000)
    sq, rq = ref.expected(rows, 3, 5, queries=[200, 7, 7])
    full = E.expected_topk(ref.scores[S.NQ_MAX][[200, 7, 7]], member, 5, None if ref.qn2 is None else ref.qn2[[200, 7, 7]])
    assert E.mismatch(sq, rq, *full) == ""
    s, r = ref.expected(rows[:3], 4, 5)
    pad = np.float32(np.inf if metric == "l2" else -np.inf)
    assert (r[:, 3:] == -1).all() and (s[:, 3:] == pad).all() and (r[:, :3] >= 0).all()
    s, r = ref.expected(np.empty(0, np.int64), 4, 5)
    assert (r == -1).all() and (s == pad).all()


def test_the_queries_of_the_k_order_test_return_distinct_rows_whose_natural_order_sum_differs():
    """the GPU test's population, on the reference alone: no query of S.PIN_QUERIES is aimed at a cluster or is the zero query, its 32
    best rows of the 2-tile list have 32 different scores, and for most of them the natural-order sum has other bits than the chain"""
    length = S.class_lengths(128)["t2"]
    span = S.span_of(length, 384)
    rows = S.make_list(length, span, 256)
    assert S.subset_plan(length, 32, 32, 384)["tiles_per_chunk"] == 2 and S.subset_plan(length, 32, 32, 384)["config"] == "S_w1_k0"
    lo, hi = S.PIN_QUERIES
    assert hi - lo == 32 and lo >= len(E.flood_layout()) and not lo <= E.ZERO_QUERY < hi
    x, q = E.corpus("random", 384, span)
    c = E.chain(q[lo:hi], x[rows], 384)
    nat = E.cflat.chain_scores(q[lo:hi], x[rows], 384, natural=True)
    es, ep = E.expected_topk(c, None, 32)
    assert all(len(set(E.bits(es[i]).tolist())) >= 31 for i in range(32)), "a query returns many copies of one score"
    assert (E.bits(np.take_along_axis(nat, ep, axis=1)) != E.bits(es)).mean() > 0.5
