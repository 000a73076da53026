"""The top-k merge's dispatch and its numpy restatement, guarded without a GPU.

tests/merge_regimes.py restates the key codec, the launcher's dispatch (which kernel, which instantiation, how many waves per query) and
the merges themselves; tests/test_merge_regimes_gpu.py runs its case table on the device.  Here:
  * the codec round-trips and orders keys as (score descending, row ascending), the empty slot below every key;
  * every constant `route()` restates is read back out of ragmeup_amd/csrc/topk_merge.hip -- a rework that moves a threshold fails
    here, naming it, and the case table has to follow;
  * CASES reaches every value of `route()` and every threshold from both sides, the candidate count of the selection kernel on both
    sides of CAPM included;
  * both references reproduce the fp64 oracle: merging per-shard `oracle.flat_search` lists gives the search over the whole corpus;
  * librmu.so exports the three launchers under the names the GPU tests call.
"""
import os
import re

import numpy as np
import pytest

from oracle import oracle as O
from tests import merge_regimes as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_STALE = "the merge dispatch moved: update tests/merge_regimes.py (route() and the CASES table) so that the GPU cases follow"


def _read(rel):
    with open(os.path.join(ROOT, rel), encoding="utf-8") as f:
        return re.sub(r"\s+", " ", f.read())


def _src():
    return _read("ragmeup_amd/csrc/topk_merge.hip")


def _hdr():
    return _read("include/rmu.h")


# ---- codec ---------------------------------------------------------------------------------------------------------------------------
def _codec_values():
    rng = np.random.default_rng(5)
    fmax, tiny = np.finfo(np.float32).max, np.float32(1e-45)              # the largest finite value, the smallest denormal
    special = np.array([0.0, -0.0, np.inf, -np.inf, fmax, -fmax, tiny, -tiny, np.float32(1.17e-38), np.float32(-1.17e-38), 1.0, -1.0], np.float32)
    s = np.concatenate([special, rng.standard_normal(300).astype(np.float32), (rng.standard_normal(100) * 1e30).astype(np.float32),
                        (rng.standard_normal(100) * 1e-41).astype(np.float32)])
    rows = np.array([0, 1, 2 ** 31 - 1, 2 ** 31, 2 ** 32 - 2], np.int64)
    return s, rows


def test_codec_round_trip_and_order():
    s, rows = _codec_values()
    assert (np.abs(s[np.isfinite(s) & (s != 0)]) < 1e-38).any() and np.isinf(s).any()
    assert np.array_equal(M.ord2f(M.f2ord(s)).view(np.uint32), s.view(np.uint32))          # bit patterns: -0 stays -0
    ss, rr = np.repeat(s, rows.size), np.tile(rows, s.size)
    keys = M.make_key(ss, rr)
    assert keys.dtype == np.uint64 and (keys != 0).all()                                    # key 0 is below every real key
    assert np.array_equal(M.key_score(keys).view(np.uint32), ss.view(np.uint32)) and np.array_equal(M.key_row(keys).astype(np.int64), rr)
    # descending key order == (score descending, row ascending); the ordinal separates -0 from +0 (-0 below)
    bits = ss.view(np.uint32).astype(np.int64)
    total = np.where(bits >> 31, -(bits & 0x7FFFFFFF) - 1, bits)                            # IEEE total order of the finite / infinite values
    want = np.lexsort((rr, -total))
    got = np.argsort(keys, kind="stable")[::-1]
    assert np.array_equal(keys[got], keys[want])
    assert np.unique(keys).size == np.unique(np.stack([ss.view(np.uint32).astype(np.int64), rr]), axis=1).shape[1]
    a, b = M.make_key(np.float32(1.5), 7), M.make_key(np.float32(1.5), 8)
    assert a > b > M.make_key(np.float32(1.25), 0) > M.make_key(np.float32(-0.0), 0) and M.make_key(np.float32(0.0), 5) > M.make_key(np.float32(-0.0), 5)
    assert (M.make_key(np.float32(-np.inf), 2 ** 32 - 2) > 0).all() and M.f2ord(np.float32(-np.inf)).tolist() == [0x007FFFFF]


# ---- the restated constants ----------------------------------------------------------------------------------------------------------
_SEL = r"if \(nq <= (\d+)\) hipLaunchKernelGGL\(\(merge_select_kernel<(\d+), (\d+)>\), dim3\(\(unsigned\)nq\), dim3\((\d+)\).*?else hipLaunchKernelGGL\(\(merge_select_kernel<(\d+), (\d+)>\), dim3\(\(unsigned\)nq\), dim3\((\d+)\)"
_REFUSE = r"if \(k < 1 \|\| k > (\d+) \|\| parts < 1 \|\| nq < 1\) return RMU_E_INVALID;"
_WPQ1 = r"while \(wpq < (\d+) && parts > (\d+) \* wpq\) wpq <<= 1;"
_WPQ2 = r"while \(wpq < (\d+) && nq \* wpq < (\d+) && wpq < parts\) wpq <<= 1;"

# name -> (where, pattern, occurrence, group, restated value)
SOURCE_CONSTANTS = {
    "key merges: k > 128 refused": (_src, _REFUSE + r" static const int use_select", 0, 1, M.MAX_K),
    "list merge: k > 128 refused": (_src, _REFUSE + r" if \(\(int64_t\)parts \* k >= \(1ll << (\d+)\)\) return RMU_E_INVALID;", 0, 1, M.MAX_K),
    "list merge: parts * k < 2^32": (_src, _REFUSE + r" if \(\(int64_t\)parts \* k >= \(1ll << (\d+)\)\) return RMU_E_INVALID;", 0, 2, 32),
    "selection: k <= 32": (_src, r"if \(use_select && k <= (\d+) && parts <= (\d+)\) \{", 0, 1, M.SELECT_SMALL_K),
    "selection, k <= 32: parts <= 1024": (_src, r"if \(use_select && k <= (\d+) && parts <= (\d+)\) \{", 0, 2, M.SELECT_MAX_PARTS),
    "selection, k > 32: parts <= 1024": (_src, r"if \(use_select && parts <= (\d+)\) \{", 0, 1, M.SELECT_MAX_PARTS),
    "k <= 32: nq <= 512": (_src, _SEL, 0, 1, M.SELECT_WIDE_NQ),
    "k <= 32, nq <= 512: BLOCK 1024": (_src, _SEL, 0, 2, M.BLOCK_WIDE),
    "k <= 32, nq <= 512: CAPM 1024": (_src, _SEL, 0, 3, M.CAPM_SMALL),
    "k <= 32, nq <= 512: 1024 threads": (_src, _SEL, 0, 4, M.BLOCK_WIDE),
    "k <= 32, nq > 512: BLOCK 256": (_src, _SEL, 0, 5, M.BLOCK_NARROW),
    "k <= 32, nq > 512: CAPM 1024": (_src, _SEL, 0, 6, M.CAPM_SMALL),
    "k <= 32, nq > 512: 256 threads": (_src, _SEL, 0, 7, M.BLOCK_NARROW),
    "k > 32: nq <= 512": (_src, _SEL, 1, 1, M.SELECT_WIDE_NQ),
    "k > 32, nq <= 512: BLOCK 1024": (_src, _SEL, 1, 2, M.BLOCK_WIDE),
    "k > 32, nq <= 512: CAPM 3072": (_src, _SEL, 1, 3, M.CAPM_DEEP),
    "k > 32, nq <= 512: 1024 threads": (_src, _SEL, 1, 4, M.BLOCK_WIDE),
    "k > 32, nq > 512: BLOCK 256": (_src, _SEL, 1, 5, M.BLOCK_NARROW),
    "k > 32, nq > 512: CAPM 3072": (_src, _SEL, 1, 6, M.CAPM_DEEP),
    "k > 32, nq > 512: 256 threads": (_src, _SEL, 1, 7, M.BLOCK_NARROW),
    "MAXP": (_src, r"constexpr int MAXP = (\d+); __shared__ u64 heads\[MAXP\];", 0, 1, M.MAXP),
    "wpq, first loop: up to 16": (_src, _WPQ1, 0, 1, M.WG_WAVES),
    "wpq, first loop: 16 parts per wave": (_src, _WPQ1, 0, 2, M.WG_PARTS_PER_WAVE),
    "wpq, second loop: up to 16": (_src, _WPQ2, 0, 1, M.WG_WAVES),
    "wpq, second loop: 2048 waves": (_src, _WPQ2, 0, 2, M.WG_MIN_WAVES),
    "queries per workgroup: 16 / wpq (launcher)": (_src, r"const int qpb = (\d+) / wpq; const dim3 grid", 0, 1, M.WG_WAVES),
    "queries per workgroup: 16 / wpq (kernel)": (_src, r"const int qpb = (\d+) / wpq; const int64_t q = ", 0, 1, M.WG_WAVES),
    "merge_wg_kernel: 16 LDS lists": (_src, r"__shared__ u64 lists\[(\d+)\]\[(\d+) \* NPL\];", 0, 1, M.WG_WAVES),
    "merge_wg_kernel: 64 keys per NPL": (_src, r"__shared__ u64 lists\[(\d+)\]\[(\d+) \* NPL\];", 0, 2, M.BATCH),
    "merge_wg_kernel: NPL = 1 up to k = 64": (_src, r"if \(k <= (\d+)\) hipLaunchKernelGGL\(merge_wg_kernel<1>, .*?else hipLaunchKernelGGL\(merge_wg_kernel<2>", 0, 1, M.NPL1_MAX_K),
    "merge_lists_kernel: NPL = 1 up to k = 64": (_src, r"if \(k <= (\d+)\) hipLaunchKernelGGL\(merge_lists_kernel<1>, .*?else hipLaunchKernelGGL\(merge_lists_kernel<2>", 0, 1, M.NPL1_MAX_K),
    "merge_stream: batches of 64": (_src, r"for \(int64_t b0 = 0; b0 < m; b0 \+= (\d+)\)", 0, 1, M.BATCH),
    "prefetched slabs: batches of 64": (_src, r"int ns0 = s0, nb0 = b0 \+ (\d+); if \(nb0 >= m\) \{ nb0 = 0; ns0 = s0 \+ (\d+); \}", 0, 1, M.BATCH),
    "prefetched slabs: 4 ranks": (_src, r"int ns0 = s0, nb0 = b0 \+ (\d+); if \(nb0 >= m\) \{ nb0 = 0; ns0 = s0 \+ (\d+); \}", 0, 2, M.SLAB),
    "prefetched slabs: 4 entries per part": (_src, r"const int m = np \* (\d+); if \(m <= 0\) return;", 0, 1, M.SLAB),
    "selection: 4 ranks per slab": (_src, r"for \(int s0 = 0; s0 < k; s0 \+= (\d+)\) \{ const int pos = s0 \+ \(lane & (\d+)\);", 0, 1, M.SLAB),
    "selection: lane & 3": (_src, r"for \(int s0 = 0; s0 < k; s0 \+= (\d+)\) \{ const int pos = s0 \+ \(lane & (\d+)\);", 0, 2, M.SLAB - 1),
    "selection: 16 parts per wave and slab": (_src, r"for \(int pb = w \* (\d+); pb < parts; pb \+= NW \* (\d+)\)", 0, 1, M.BATCH // M.SLAB),
    "selection: 16 parts per wave and slab (step)": (_src, r"for \(int pb = w \* (\d+); pb < parts; pb \+= NW \* (\d+)\)", 0, 2, M.BATCH // M.SLAB),
    "RMU_E_INVALID": (_hdr, r"#define RMU_E_INVALID \((-?\d+)\)", 0, 1, M.E_INVALID),
}

SOURCE_SHAPES = {
    "the switch is RMU_MERGE_SELECT, default on": r'static const int use_select = rmu_env\("RMU_MERGE_SELECT"\) \? atoi\(rmu_env\("RMU_MERGE_SELECT"\)\) : 1;',
    "branch order: selection k <= 32, selection, merge_wg_kernel": r"if \(use_select && k <= \d+ && parts <= \d+\) \{.*?\} if \(use_select && parts <= \d+\) \{.*?\} // waves per query",
    "the fallback: count > CAPM, never at k <= 32": r"if \(CAPM < 128 \* 128 && count > \(u32\)CAPM\) \{",
    "selection: keys >= tau": r"const bool take = key != 0ull && key >= tau;",
    "tau only when parts >= k": r"if \(parts >= k\) \{ for \(int p = tid; p < parts; p \+= BLOCK\) \{ const u64 mine = heads\[p\];",
    "unsorted: only an empty slab ends a part": r"if \(o\.unsorted && __ballot\(key != 0ull\)\) continue;",
    "seed_thr: the k-th key, unless it is the sentinel": r"if \(o\.seed_thr && e == k - 1 && key\) atomicMax\(o\.seed_thr \+ qo, \(u32\)\(key >> 32\)\);",
    "l2_out: qnorm2 by the output row": r"if \(o\.l2_out\) sc = fmaxf\(o\.qnorm2\[qo\] - sc, 0\.f\);",
    "cond: outside -> nothing, clamp -> c queries": r"if \(c < cond\.lo \|\| c > cond\.hi\) return; // uniform over the grid if \(cond\.clamp && c < nq_eff\) nq_eff = c;",
    "list merge: row < 0 or NaN dropped, zeros canonical": r"if \(rows\[part \* stride_r \+ q \* k \+ pos\] < 0 \|\| !\(s == s\)\) return 0ull; return rmu_make_key\(\(smaller_better \? -s : s\) \+ 0\.0f, \(u32\)idx\);",
    "list merge: a zero distance comes out as +0": r"out_scores\[q \* k \+ e\] = smaller_better \? 0\.0f - rmu_key_score\(key\) : rmu_key_score\(key\);",
}


@pytest.mark.parametrize("name", list(SOURCE_CONSTANTS))
def test_constant_matches_the_source(name):
    where, pat, nth, group, want = SOURCE_CONSTANTS[name]
    found = list(re.finditer(pat, where()))
    assert len(found) > nth, f"{name}: pattern not found in the source -- {_STALE}"
    got = int(found[nth].group(group))
    assert got == want, f"{name}: the source says {got}, tests/merge_regimes.py says {want} -- {_STALE}"


@pytest.mark.parametrize("name", list(SOURCE_SHAPES))
def test_dispatch_shape_matches_the_source(name):
    assert re.search(SOURCE_SHAPES[name], _src()), f"{name}: not found in the source -- {_STALE}"


def test_route_restates_the_launcher():
    assert M.route(1, 1, 1) == ("select", 1024, 1024) and M.route(1024, 512, 32) == ("select", 1024, 1024)
    assert M.route(1024, 513, 32) == ("select", 256, 1024) and M.route(1024, 512, 33) == ("select", 1024, 3072)
    assert M.route(7, 513, 128) == ("select", 256, 3072) and M.route(1025, 513, 10) == ("wg", 1, 16) and M.route(1025, 1, 65) == ("wg", 2, 16)
    assert [M.route(*a)[0] for a in ((1, 1, 0), (1, 1, 129), (0, 1, 5), (1, 0, 5))] == ["invalid"] * 4
    w = lambda parts, nq: M.route(parts, nq, 10, select=False)[2]
    assert [w(16, 2048), w(16, 2047), w(17, 1024), w(17, 1023), w(33, 512), w(65, 256), w(129, 10 ** 6)] == [1, 2, 2, 4, 4, 8, 16]
    assert [w(1, 1), w(2, 1), w(3, 1), w(4, 1), w(5, 1), w(8, 1), w(9, 1), w(1040, 3)] == [1, 2, 4, 4, 8, 8, 16, 16]
    assert M.route(3, 5, 64, select=False) == ("wg", 1, 4) and M.route(3, 5, 65, select=False) == ("wg", 2, 4)


# ---- coverage ----------------------------------------------------------------------------------------------------------------------
def _cap_side(case):
    cnt = M.count_ge_tau(M.build(case).lists, case.k)
    capm = case.route[2]
    return "over" if (cnt > capm).any() else ("at" if (cnt == capm).any() else ""), cnt


def test_cases_reach_every_route_and_every_threshold_from_both_sides():
    ids = [c.id for c in M.CASES]
    assert len(ids) == len(set(ids))
    sorted_cases = [c for c in M.CASES if not c.unsorted]
    # every value of route() in the default process ...
    want = {("select", b, m) for b in (1024, 256) for m in (1024, 3072)} | {("wg", 1, 16), ("wg", 2, 16)}
    for group in (sorted_cases, [c for c in M.CASES if c.unsorted and c.nq <= 512]):
        have = {c.route for c in group}
        assert want - {("select", 256, 1024), ("select", 256, 3072)} <= have, sorted(want - have)
    assert want == {c.route for c in sorted_cases}
    assert ("select", 256, 1024) in {c.route for c in M.CASES if c.unsorted}
    # ... and with the selection switched off: merge_wg_kernel at every wpq, in both NPL
    assert {c.route_wg for c in M.CASES} >= {("wg", npl, w) for npl in (1, 2) for w in (1, 2, 4, 8, 16)}
    assert all(c.route_wg[0] == "wg" for c in M.CASES)
    shapes = {(c.parts, c.nq, c.k) for c in sorted_cases}
    ks, ps, nqs = {s[2] for s in shapes}, {s[0] for s in shapes}, {s[1] for s in shapes}

    def both(pred_lo, pred_hi):
        return any(pred_lo(*s) for s in shapes) and any(pred_hi(*s) for s in shapes)

    # the dispatch thresholds
    assert both(lambda p, n, k: k == 32 and p <= 1024, lambda p, n, k: k == 33 and p <= 1024)
    assert both(lambda p, n, k: p == 1024 and k <= 32, lambda p, n, k: p == 1025 and k <= 32)
    assert both(lambda p, n, k: p == 1024 and k > 32, lambda p, n, k: p == 1025 and k > 32)
    assert both(lambda p, n, k: n == 512 and k <= 32, lambda p, n, k: n == 513 and k <= 32)
    assert any(n == 513 and k > 32 for p, n, k in shapes) and any(n <= 512 and k > 32 for p, n, k in shapes)
    assert both(lambda p, n, k: k == 64 and p > 1024, lambda p, n, k: k == 65 and p > 1024) and 128 in ks and max(ks) == M.MAX_K
    assert (0, 4, 3) in M.REFUSED and (129, 4, 3) in M.REFUSED and any(p == 0 for _, p, _ in M.REFUSED) and any(n == 0 for _, _, n in M.REFUSED)
    # the two wpq loops: parts = 16 * wpq | + 1 with queries to spare, nq * wpq around 2048, wpq against parts
    for lo, hi, nq in ((16, 17, 1024), (32, 33, 64), (64, 65, 32), (128, 129, 16)):
        a = [s for s in shapes if s[0] == lo and s[1] >= nq]
        b = [s for s in shapes if s[0] == hi and s[1] >= nq]
        assert a and b, (lo, hi)
    assert M.wpq_of(16, 2048) == 1 and M.wpq_of(16, 2047) == 2 and {(16, 2048, 3), (16, 2047, 3)} <= shapes
    assert M.wpq_of(2, 5) == 2 and M.wpq_of(3, 5) == 4 and {(2, 5, 65), (3, 5, 65)} <= shapes
    # tau: parts == k, k - 1, k + 1, parts < k, at k <= 32 and above; parts == 1
    for small in (True, False):
        rel = {p - k for p, n, k in shapes if (k <= 32) == small and p <= 1024}
        assert {-1, 0, 1} <= rel and min(rel) < -1 and max(rel) > 1, rel
    assert 1 in ps and {1, 5, 512, 513} <= nqs and {1, 3, 10, 31, 32, 33, 64, 65, 100, 127, 128} <= ks
    # guards: k not a multiple of the slab, parts not a multiple of 16 (the batch holds 16 parts), the 32 / 33 and 64 / 65 seams
    assert any(k % M.SLAB for k in ks) and any(p % 16 for p in ps) and any(p % 16 == 0 for p in ps) and {17, 250, 1024, 1025, 1040} <= ps
    # fills: sparse lists, queries without a key, fewer than k heads among parts >= k, one sub wave, fewer than k keys in all
    assert {"full", "sparse", "mixed", "lens", "wg"} <= {c.fill for c in M.CASES}
    b = M.build(next(c for c in M.CASES if c.id == "sel-k10-p250-nq5-sparse"))
    heads = (b.lists != 0).any(axis=2).sum(axis=0)
    assert heads[1] == 0 and heads[2] == 9 and (M.count_ge_tau(b.lists, 10)[2] == (b.lists[:, 2] != 0).sum())
    b = M.build(next(c for c in M.CASES if c.id == "wg-k64-p1040-nq3-wg"))
    occupied = np.nonzero((b.lists[:, 0] != 0).any(axis=1))[0]
    assert occupied.size and (occupied % 16 == 5).all() and 0 < (b.lists[:, 1] != 0).sum() < 64
    # MergeOut: each field on a selection case and on a merge_wg case
    for kind in ("select", "wg"):
        cs = [c for c in M.CASES if c.route[0] == kind]
        assert any(c.row_base for c in cs) and any(c.scatter for c in cs) and any(c.l2 for c in cs) and any(c.scatter and c.l2 for c in cs)
        conds = [c.cond for c in cs if c.cond]
        assert any(c < lo for c, lo, hi, cl in conds) and any(c > hi for c, lo, hi, cl in conds)
        assert any(lo <= c <= hi and cl and c < 6 for c, lo, hi, cl in conds) and any(lo <= c <= hi and not cl for c, lo, hi, cl in conds)
        assert any(c == lo for c, lo, hi, cl in conds) and any(c == hi for c, lo, hi, cl in conds)
    # unsorted: lists of 1, 4, 5 and k keys, k in {10, 32, 40, 128}, the overflow pair, parts beyond 1024
    us = [c for c in M.CASES if c.unsorted]
    assert {10, 32, 40, 128} <= {c.k for c in us} and any(c.fill == "lens" for c in us) and any(c.parts > 1024 for c in us)
    assert {"at", "over"} <= {c.cap for c in us}


@pytest.mark.parametrize("case", [c for c in M.CASES if c.route[0] == "select"], ids=lambda c: c.id)
def test_candidate_count_of_the_case_lies_on_its_side_of_capm(case):
    side, cnt = _cap_side(case)
    if case.route[2] == M.CAPM_SMALL:
        assert side in ("", "at") and case.cap == "", (case.id, int(cnt.max()))          # k parts x k keys: the array cannot overflow
    else:
        assert side == case.cap, (case.id, side, int(cnt.max()))


def test_both_sides_of_capm_are_held_exactly():
    by = {c.id: c for c in M.CASES}
    for tag in ("deep", "unsorted"):
        at, over = by[f"{tag}-k128-p24-count3072"], by[f"{tag}-k128-p25-count3073"]
        assert M.count_ge_tau(M.build(at).lists, 128).tolist() == [3072, 3072]
        assert M.count_ge_tau(M.build(over).lists, 128).tolist() == [3073, 3072]
    low = M.build(by["deep-k128-p128-tau-low"]).lists
    assert (M.count_ge_tau(low, 128) == 127 * 128 + 1).all()                                # tau is the single low key of the last part
    for q in range(2):
        nz = low[:, q][low[:, q] != 0]
        assert low[-1, q, 0] == nz.min() and (low[-1, q, 1:] == 0).all()
    assert 0 < int(M.count_ge_tau(M.build(by["deep-k128-p130-nq2-full"]).lists, 128).max()) < M.CAPM_DEEP // 2


def test_builders_keep_their_promises():
    rng = np.random.default_rng(3)
    counts = rng.integers(0, 11, (7, 4))
    for unsorted in (False, True):
        lists = M.build_lists(7, 4, 10, counts, np.random.default_rng(9), unsorted=unsorted, ties=True)
        assert lists.shape == (7, 4, 10) and lists.dtype == np.uint64 and np.array_equal((lists != 0).sum(axis=2), counts)
        for q in range(4):
            nz = lists[:, q][lists[:, q] != 0]
            assert np.unique(nz).size == nz.size                                           # distinct keys within a query
        for p in range(7):
            for q in range(4):
                c, l = counts[p, q], lists[p, q]
                assert (l[:c] != 0).all() and (l[c:] == 0).all()                          # compact, zeros last
                if not unsorted:
                    assert (np.diff(l[:c].astype(object)) < 0).all()
                elif c:
                    assert l[c - 1] == l.max()                                             # the best key in the last occupied slot
    big = M.build_lists(3, 2, 5, np.full((3, 2), 5), np.random.default_rng(1))
    assert (M.key_row(big).astype(np.int64) == 2 ** 32 - 2).any() and (M.key_row(big) == 0).any()
    shuffled = [c for c in M.CASES if c.unsorted and c.k >= 10]
    assert any((np.diff(M.build(c).lists[:, :, :4].astype(np.float64), axis=2) > 0).any() for c in shuffled[:2])
    for c in M.CASES:
        assert c.parts * c.nq * c.k * 8 <= 3_400_000, c.id                                 # a few MB at most


# ---- the references against the oracle --------------------------------------------------------------------------------------------------
def test_references_reproduce_the_search_over_the_whole_corpus():
    x = O.make_corpus(900, seed=11)
    q, _ = O.make_queries(x, 9, seed=12)
    k = 10
    ps, pr = [], []
    for lo in list(range(0, 750, 150)) + [750, 897]:                   # five shards of 150, one of 147 and one of 3 rows (a short list)
        hi = {750: 897, 897: 900}.get(lo, lo + 150)
        s, r = O.flat_search(q, x[lo:hi], k)
        ps.append(s.astype(np.float32))
        pr.append(np.where(r >= 0, r + lo, -1))
    ps, pr = np.stack(ps), np.stack(pr)
    gs, gr = O.flat_search(q, x, k)
    ms, mr, mi = M.ref_lists(ps, pr, k, False)
    assert np.array_equal(mr, gr) and np.array_equal(ms, gs.astype(np.float32)) and (mi >= 0).all()
    ds, dr, _ = M.ref_lists(-ps, pr, k, True)                            # the same lists as distances
    assert np.array_equal(dr, gr) and np.array_equal(ds, -gs.astype(np.float32))
    keys = np.where(pr >= 0, M.make_key(ps, np.maximum(pr, 0)), np.uint64(0))
    bits, rows = M.ref_final(keys, k)
    assert np.array_equal(rows, gr) and np.array_equal(bits, gs.astype(np.float32).view(np.uint32))
    os_, or_ = O.merge_topk(ps, pr, k)
    assert np.array_equal(rows, or_) and np.array_equal(bits.view(np.float32), os_.astype(np.float32))
    # ... with equal scores in different shards (the oracle orders them by row, the keys do too), and fewer than k candidates
    ps2 = (np.round(ps * 8) / 8).astype(np.float32)
    keys2 = np.where(pr >= 0, M.make_key(ps2, np.maximum(pr, 0)), np.uint64(0))
    bits2, rows2 = M.ref_final(keys2, k, row_base=5)
    os2, or2 = O.merge_topk(ps2, pr, k)
    assert np.array_equal(rows2, or2 + 5) and np.array_equal(bits2.view(np.float32), os2.astype(np.float32))
    bits3, rows3 = M.ref_final(keys[6:], k)                              # the 3-row shard alone
    assert (rows3[:, 3:] == -1).all() and (bits3[:, 3:].view(np.float32) == -np.inf).all() and (rows3[:, :3] >= 897).all()


def test_reference_semantics_of_merge_out():
    case = next(c for c in M.CASES if c.id == "out-sel-scatter-l2-rowbase")
    b = M.build(case)
    bits, rows = M.ref_final(b.lists, case.k, row_base=case.row_base, l2_out=True, qn=b.qn, scatter=b.scatter, n_out=b.n_out)
    untouched = np.setdiff1d(np.arange(b.n_out), b.scatter)
    assert untouched.size == 3 and (bits[untouched] == M.FILL_BITS).all() and (rows[untouched] == M.FILL_ROW).all()
    plain_bits, plain_rows = M.ref_final(b.lists, case.k)
    s = plain_bits.view(np.float32)
    want = np.maximum(b.qn[b.scatter][:, None] - s, np.float32(0))
    want = np.where(plain_rows < 0, np.float32(np.inf), want)
    assert np.array_equal(bits[b.scatter].view(np.float32), want) and (want == 0).any() and (want[np.isfinite(want)] > 0).any()   # the clamp acts
    assert np.array_equal(rows[b.scatter], np.where(plain_rows < 0, -1, plain_rows + case.row_base))
    # cond
    for cond, n_written in (((2, 3, 6, 1), 0), ((7, 3, 6, 1), 0), ((3, 3, 6, 1), 3), ((5, 1, 5, 1), 5), ((2, 1, 0x7FFFFFFF, 0), 6)):
        _, r = M.ref_final(b.lists, case.k, cond=cond)
        assert ((r != M.FILL_ROW).any(axis=1)).sum() == n_written and ((r != M.FILL_ROW).any(axis=1))[:n_written].all()
    # seed_thr: above stays, below is raised, equal stays, an empty k-th slot leaves it alone
    keys, seed = M.ref_to_keys(b.lists, case.k, b.seed_init)
    kth = (keys[:, -1] >> np.uint64(32)).astype(np.uint32)
    assert (kth != 0).all() and seed.tolist() == [int(kth[0]) + 1, int(kth[1]), int(kth[2]), int(kth[3]), int(kth[4]) + 1, int(kth[5])]
    sparse = M.build(next(c for c in M.CASES if c.id == "sel-k10-p250-nq5-sparse"))
    keys, seed = M.ref_to_keys(sparse.lists, 10, np.full(5, 77, np.uint32))
    assert (keys[1] == 0).all() and seed[1] == 77 and seed[0] == max(77, int(keys[0, -1] >> np.uint64(32)))


def test_list_cases_hold_what_they_are_there_for():
    assert {c.k for c in M.LIST_CASES} == {1, 10, 64, 65, 128} and {c.parts for c in M.LIST_CASES} == {1, 2, 8, 13}
    assert {c.nq for c in M.LIST_CASES} == {1, 4, 7} and {c.layout for c in M.LIST_CASES} == {"packed", "padded", "comm"}
    assert {(c.smaller_better, c.k > 64) for c in M.LIST_CASES} == {(a, b) for a in (False, True) for b in (False, True)}
    assert any(c.parts * c.k % 64 == 0 for c in M.LIST_CASES) and any(c.parts * c.k % 64 for c in M.LIST_CASES)
    seen = set()
    for c in M.LIST_CASES:
        s, r = M.build_list_case(c)
        os_, or_, oi = M.ref_lists(s, r, c.k, c.smaller_better)
        valid = (r >= 0) & ~np.isnan(s)
        assert not np.isnan(os_).any() and ((or_ >= 0) == (oi >= 0)).all()
        for q in range(c.nq):
            n = min(c.k, int(valid[:, q].sum()))
            assert (or_[q, :n] >= 0).all() and (or_[q, n:] == -1).all() and (os_[q, n:] == (np.inf if c.smaller_better else -np.inf)).all()
            with np.errstate(invalid="ignore"):
                d = np.diff(os_[q, :n].astype(np.float64))
            assert ((d >= 0) if c.smaller_better else (d <= 0))[~np.isnan(d)].all()
            same = np.nonzero(d == 0)[0] if n > 1 else []
            assert all(oi[q, i] < oi[q, i + 1] for i in same)                             # equal scores: lower part, then earlier position
            if len(same) and any(oi[q, i] // c.k != oi[q, i + 1] // c.k for i in same):
                seen.add("tie across parts")
            if len(same) and any(oi[q, i] // c.k == oi[q, i + 1] // c.k for i in same):
                seen.add("tie inside a part")
        kept = os_[or_ >= 0]
        seen |= {name for name, hit in (("zero", (kept == 0).any()), ("+inf kept", np.isposinf(kept).any()), ("-inf kept", np.isneginf(kept).any()),
                                        ("NaN beside a row", (np.isnan(s) & (r >= 0)).any()), ("-0 in", ((s == 0) & np.signbit(s) & (r >= 0)).any()),
                                        ("empty query", (or_ == -1).all(axis=1).any()), ("short", ((or_ == -1).any(axis=1) & (or_ >= 0).any(axis=1)).any())) if hit}
        bufs, off_s, off_r, ss, sr = M.lay_out(c, s, r)
        assert ss >= c.nq * c.k and sr >= c.nq * c.k and (c.layout == "packed") == (ss == c.nq * c.k == sr)
    assert seen == {"tie across parts", "tie inside a part", "zero", "+inf kept", "-inf kept", "NaN beside a row", "-0 in", "empty query", "short"}, seen


# ---- the exported launchers ---------------------------------------------------------------------------------------------------------
def test_the_three_launchers_resolve(librmu):
    fns = M.launchers(librmu)
    assert set(fns) == {"final", "to_keys", "lists"} and all(f.restype is not None for f in fns.values())
