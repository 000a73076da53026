"""The MMR selection's dispatch, its exact host reference and its case table, guarded without a GPU.

tests/mmr_regimes.py restates launch_mmr's dispatch, holds the reference (`ref_mmr`: exact products, math.fsum) and the table of cases
tests/test_mmr_regimes_gpu.py runs on the device.  Here:
  * every constant the module restates is read back out of ragmeup_amd/csrc/rmu_api.hip and include/rmu.h -- a rework that moves a
    threshold fails here, naming it, and the case table has to follow;
  * CASES reaches both kernels from both sides of both thresholds, every remainder of k_mmr_lds's unrolled chain, every fill of k_mmr's
    last workgroup, and every list and data class, by name and by content;
  * EVERY decision of EVERY case is settled: its margin is at least MARGIN_MIN, or it is an exact tie inside one constructed class -- the
    share of decisions left out of the comparison is zero, so the GPU test may compare picks by equality;
  * the reference is right: worked examples, and the fp64 oracle (`oracle.mmr`, numpy BLAS) on every case without absent candidates;
  * the removed-row cases tell the contract (a removed row is absent) from what a kernel does that reads the NaN row as cosine 0.
"""
import os
import re

import numpy as np
import pytest

from oracle import oracle as O
from tests import mmr_regimes as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_STALE = "the MMR dispatch moved: update tests/mmr_regimes.py (route() and the CASES table) so that the GPU cases follow"


def _read(rel):
    with open(os.path.join(ROOT, rel), encoding="utf-8") as f:
        return re.sub(r"\s+", " ", f.read())


def _src():
    return _read("ragmeup_amd/csrc/rmu_api.hip")


def _hdr():
    return _read("include/rmu.h")


# ---- the restated constants ----------------------------------------------------------------------------------------------------------
_DISPATCH = r"if \(idx->dim <= (\d+) && nq <= (\d+) && !lds_off\) \{"
_LDS_SIZE = r"const size_t lds = \(size_t\)\((\d+) \* (\d+) \+ (\d+)\) \* sizeof\(float\) \+ \(size_t\)\((\d+) \* (\d+) \+ (\d+)\) \* sizeof\(double\);"
_LDS_ATTR = r"hipFuncAttributeMaxDynamicSharedMemorySize, \((\d+) \* (\d+) \+ (\d+)\) \* (\d+) \+ \((\d+) \* (\d+) \+ (\d+)\) \* (\d+)\);"
_WAVE_LAUNCH = r"hipLaunchKernelGGL\(k_mmr, dim3\(\(unsigned\)\(\(nq \+ (\d+)\) / (\d+)\)\), dim3\((\d+)\), 0, s,"
_LDS_LAUNCH = r"hipLaunchKernelGGL\(k_mmr_lds, dim3\(\(unsigned\)nq\), dim3\((\d+)\), lds, s,"
_TAIL = r"for \(int t = want \+ lane; t < k; t \+= (\d+)\) out_pos\[qi \* k \+ t\] = -1;"
_CHAIN = r"for \(; c \+ (\d+) <= dim; c \+= (\d+)\) \{ s0 = fma"
_G = r"double\* G = \(double\*\)\(mm \+ (\d+) \* (\d+) \+ (\d+)\);"

# name -> (where, pattern, occurrence, group, restated value)
SOURCE_CONSTANTS = {
    "k_mmr_lds up to dim 384": (_src, _DISPATCH, 0, 1, M.LDS_MAX_DIM),
    "k_mmr_lds up to 65535 queries": (_src, _DISPATCH, 0, 2, M.LDS_MAX_NQ),
    "rmu_index_mmr: fetch_k <= 64": (_src, r"fetch_k > (\d+) \|\| k < 1\) return rmu_fail\(RMU_E_INVALID, \"rmu_index_mmr:", 0, 1, M.MAX_FETCH_K),
    "rmu_index_search_mmr: fetch_k <= 64": (_src, r"fetch_k > (\d+) \|\| k < 1 \|\| k > fetch_k\) return rmu_fail\(RMU_E_INVALID, \"rmu_index_search_mmr:", 0, 1, M.MAX_FETCH_K),
    "rmu.h: fetch_k <= 64": (_hdr, r"RMU_F_OUT_DEVICE \(rows and out_pos\)\. fetch_k <= (\d+)\.", 0, 1, M.MAX_FETCH_K),
    "k_mmr: 4 queries per workgroup (kernel)": (_src, r"const int64_t qi = \(int64_t\)blockIdx\.x \* (\d+) \+ \(threadIdx\.x >> 6\);", 0, 1, M.WAVE_QUERIES_PER_WG),
    "k_mmr: 4 queries per workgroup (grid, rounding)": (_src, _WAVE_LAUNCH, 0, 1, M.WAVE_QUERIES_PER_WG - 1),
    "k_mmr: 4 queries per workgroup (grid)": (_src, _WAVE_LAUNCH, 0, 2, M.WAVE_QUERIES_PER_WG),
    "k_mmr: 4 waves per workgroup": (_src, _WAVE_LAUNCH, 0, 3, 64 * M.WAVE_QUERIES_PER_WG),
    "k_mmr_lds: 256 threads": (_src, _LDS_LAUNCH, 0, 1, 256),
    "k_mmr: the -1 fill strides by 64": (_src, _TAIL, 0, 1, M.TAIL_STRIDE),
    "k_mmr_lds: the -1 fill strides by 64": (_src, _TAIL, 1, 1, M.TAIL_STRIDE),
    "k_mmr_lds: 4 chains (bound)": (_src, _CHAIN, 0, 1, M.LDS_UNROLL),
    "k_mmr_lds: 4 chains (step)": (_src, _CHAIN, 0, 2, M.LDS_UNROLL),
    "LDS area: 64 rows": (_src, _LDS_SIZE, 0, 1, M.MAX_FETCH_K),
    "LDS area: rows of 385 floats": (_src, _LDS_SIZE, 0, 2, M.LDS_MAX_DIM + 1),
    "LDS area: a query of 384 floats": (_src, _LDS_SIZE, 0, 3, M.LDS_MAX_DIM),
    "LDS area: 65 Gram rows": (_src, _LDS_SIZE, 0, 4, M.MAX_FETCH_K + 1),
    "LDS area: Gram rows of 64": (_src, _LDS_SIZE, 0, 5, M.MAX_FETCH_K),
    "kernel: the Gram block behind 64 rows": (_src, _G, 0, 1, M.MAX_FETCH_K),
    "kernel: ... of 385 floats": (_src, _G, 0, 2, M.LDS_MAX_DIM + 1),
    "kernel: ... and the query": (_src, _G, 0, 3, M.LDS_MAX_DIM),
    "RMU_F_Q_DEVICE": (_hdr, r"#define RMU_F_Q_DEVICE (\d+)u", 0, 1, M.F_Q_DEVICE),
    "RMU_F_OUT_DEVICE": (_hdr, r"#define RMU_F_OUT_DEVICE (\d+)u", 0, 1, M.F_OUT_DEVICE),
}

SOURCE_SHAPES = {
    "the switch is RMU_MMR_LDS, read once, off only at 0": r'static const bool lds_off = rmu_env\("RMU_MMR_LDS"\) && atoi\(rmu_env\("RMU_MMR_LDS"\)\) == 0;',
    "two arms: k_mmr_lds, else k_mmr": r"&& !lds_off\) \{.*?hipLaunchKernelGGL\(k_mmr_lds, .*?\} else \{ hipLaunchKernelGGL\(k_mmr, ",
    "ties: the lowest lane (both kernels)": r"return eq \? __builtin_ctzll\(eq\) : -1;.*return eq \? __builtin_ctzll\(eq\) : -1;",
    "redundancy: the maximum over the picked set (both kernels)": r"red = fmax\(red, cs\);.*red = fmax\(red, cs\);",
    "k_mmr: a row outside the index or with a NaN norm is absent": r"const bool in_index = row >= 0 && row < n_rows;.*?const bool valid = in_index && nx == nx;.*?__ballot\(valid\)",
    "k_mmr_lds: a row outside the index or with a NaN norm is absent": r"const bool valid = row >= 0 && row < n_rows && nx == nx;.*?__ballot\(valid\)",
    "k_mmr_lds: an absent row is staged as zeros": r"mm\[r \* ld \+ c\] = \(row >= 0 && row < n_rows\) \? x\[row \* \(int64_t\)dpad \+ c\] : 0\.f;",
    "removal poisons the row with NaN": r"for \(int c = threadIdx\.x; c < dpad; c \+= blockDim\.x\) row\[c\] = __builtin_nanf\(\"\"\);",
    "rmu.h says a removed row is absent": r"the id of a REMOVED row .*? are absent",
}


@pytest.mark.parametrize("name", list(SOURCE_CONSTANTS))
def test_constant_matches_the_source(name):
    where, pat, nth, group, want = SOURCE_CONSTANTS[name]
    found = list(re.finditer(pat, where()))
    assert len(found) > nth, f"{name}: pattern not found in the source -- {_STALE}"
    got = int(found[nth].group(group))
    assert got == want, f"{name}: the source says {got}, tests/mmr_regimes.py says {want} -- {_STALE}"


@pytest.mark.parametrize("name", list(SOURCE_SHAPES))
def test_dispatch_shape_matches_the_source(name):
    where = _hdr if name.startswith("rmu.h") else _src
    assert re.search(SOURCE_SHAPES[name], where()), f"{name}: not found in the source -- {_STALE}"


def test_lds_byte_count_matches_both_places_in_the_source():
    for pat in (_LDS_SIZE, _LDS_ATTR):
        m = re.search(pat, _src())
        assert m, _STALE
        g = [int(v) for v in m.groups()]
        if pat is _LDS_SIZE:
            g = g[:3] + [4] + g[3:] + [8]                                      # sizeof(float), sizeof(double)
        assert (g[0] * g[1] + g[2]) * g[3] + (g[4] * g[5] + g[6]) * g[7] == M.LDS_BYTES == 100096 + 33288
    assert M.LDS_BYTES <= 160 * 1024                                       # the LDS of one CDNA4 compute unit
    assert (64 * (M.LDS_MAX_DIM + 1) + M.LDS_MAX_DIM) * 4 % 8 == 0         # the fp64 block starts 8-byte aligned


def test_route_restates_the_launcher():
    assert M.route(384, 1) == "lds" and M.route(385, 1) == "wave" and M.route(1, 65535) == "lds" and M.route(1, 65536) == "wave"
    assert M.route(384, 65535) == "lds" and M.route(3072, 1) == "wave"
    assert all(M.route(d, n, lds_on=False) == "wave" for d in (1, 384, 385) for n in (1, 65535, 65536))


# ---- coverage ----------------------------------------------------------------------------------------------------------------------
def _by(route):
    return [c for c in M.CASES if c.route == route]


def test_case_table_is_well_formed():
    ids = [c.id for c in M.CASES]
    assert len(ids) == len(set(ids))
    for c in M.CASES:
        assert c.metric in ("ip", "cosine", "l2") and c.lists in M.LIST_BUILDERS and c.data in M.DATA_BUILDERS
        assert 1 <= c.n_rows <= 300 and 1 <= c.fetch_k <= M.MAX_FETCH_K and c.k >= 1 and 0.0 <= c.lam <= 1.0 and c.nq >= 1
        assert c.metric != "l2" or c.dim <= 767
        b = M.build(c)
        assert b.q.shape == (c.nq, c.dim) and b.lists.shape == (c.nq, c.fetch_k) and b.q.dtype == np.float32 and b.lists.dtype == np.int64
        assert b.data.x.shape == (c.n_rows, c.dim) and np.isfinite(b.data.x).all() and np.isfinite(b.q).all()
        if c.tile:                                                            # the tiled queries repeat with the period of the distinct ones
            assert np.array_equal(b.q[c.tile:2 * c.tile], b.q[:c.tile]) and np.array_equal(b.lists[-1], b.rows[(c.nq - 1) % c.tile])
        assert all(c.route == r for r in [M.route(c.dim, c.nq)])


def test_cases_reach_both_routes_from_both_sides_of_both_thresholds():
    key = lambda c: (c.nq, c.fetch_k, c.k, c.lam, c.lists, c.data, c.metric)
    at = {key(c) for c in M.CASES if c.dim == M.LDS_MAX_DIM and c.route == "lds"}
    over = {key(c) for c in M.CASES if c.dim == M.LDS_MAX_DIM + 1 and c.route == "wave"}
    assert at & over, "no pair of cases that differs in dim 384 | 385 alone"
    key = lambda c: (c.dim, c.fetch_k, c.k, c.lam, c.lists, c.data, c.metric)
    at = {key(c) for c in M.CASES if c.nq == M.LDS_MAX_NQ and c.route == "lds"}
    over = {key(c) for c in M.CASES if c.nq == M.LDS_MAX_NQ + 1 and c.route == "wave" and c.dim <= M.LDS_MAX_DIM}
    assert at & over, "no pair of cases that differs in nq 65535 | 65536 alone"
    assert (4, 4, 2, 0.5, "perm", "random", "ip") in at & over


def test_cases_reach_every_inner_loop_shape():
    lds, wave = _by("lds"), _by("wave")
    assert {1, 2, 3, 4, 5, 7, 383, 384} <= {c.dim for c in lds}
    assert {c.dim % M.LDS_UNROLL for c in lds} == {0, 1, 2, 3} and any(c.dim < M.LDS_UNROLL for c in lds)      # the main loop empty
    assert {1, 2, 20, 63, 64} <= {c.fetch_k for c in lds}
    assert any(c.dim == M.LDS_MAX_DIM and c.fetch_k == M.MAX_FETCH_K for c in lds)                               # the whole LDS area
    assert {385, 768, 1024, 3072} <= {c.dim for c in wave}
    assert {1, 3, 4, 5} <= {c.nq for c in wave} and {c.nq % M.WAVE_QUERIES_PER_WG for c in wave} == {0, 1, 2, 3}
    assert {1, 20, 64} <= {c.fetch_k for c in wave}
    for cs in (lds, wave):
        two = [c for c in cs if c.lists == "two_live"]
        assert {1, 70, 130} <= {c.k for c in two} and any(c.k == c.fetch_k for c in two)
        assert any(c.k - 2 > 2 * M.TAIL_STRIDE - 2 for c in two)           # the -1 fill of some lane runs more than once
        for c in two:
            assert ((M.build(c).rows >= 0).sum(axis=1) == 2).all()
        assert {0.0, 0.35, 0.5, 1.0} <= {c.lam for c in cs}
        assert {"ip", "cosine", "l2"} <= {c.metric for c in cs}
        assert any(c.metric == "cosine" and c.data == "zero_row" for c in cs)
        assert any(c.data == "removed" for c in cs)


@pytest.mark.parametrize("route", ["lds", "wave"])
def test_cases_hold_every_list_class_on_both_routes(route):
    cs = {c.lists: c for c in _by(route) if c.data == "random" and c.metric == "ip"}
    assert {"mid_absent", "head_absent", "all_absent", "stale", "repeat", "tail_absent"} <= set(cs)
    r = M.build(cs["mid_absent"]).rows
    assert all((row[0] >= 0) and (row[-1] >= 0) and (row[1:-1] == -1).any() for row in r)
    r = M.build(cs["head_absent"]).rows
    assert (r[:, 0] == -1).all() and (r[:, 2:] >= 0).all()
    r = M.build(cs["all_absent"]).rows
    assert (r[1] == -1).all() and (r[0] >= 0).all() and (r[2] >= 0).all()
    c = cs["all_absent"]
    assert (M.expect(c).picks[1] == -1).all() and (M.expect(c).picks[[0, 2]] >= 0).all()
    c = cs["stale"]
    r = M.build(c).rows
    assert all((row == c.n_rows).any() and (row > c.n_rows).any() and (row >= 2 ** 32).any() for row in r)      # the first id past the index, and far ones
    want = M.expect(c).picks
    assert (want >= 0).all() and all(0 <= r[i, p] < c.n_rows for i in range(c.distinct) for p in want[i])      # never a stale position
    r = M.build(cs["repeat"]).rows
    assert all(len(set(row.tolist())) == row.size - 1 and (row >= 0).all() for row in r)


@pytest.mark.parametrize("route", ["lds", "wave"])
def test_cases_hold_every_data_class_on_both_routes(route):
    cs = {c.data: c for c in _by(route) if c.lists == "perm" and c.metric == "ip" and c.dim > 1}
    assert {"identical", "zero_row", "zero_query", "near_dup", "pow2", "removed"} <= set(cs)
    in_every_list = lambda c, rows: all(set(rows) <= set(l.tolist()) for l in M.build(c).rows)
    d = M.build(cs["identical"]).data
    assert np.array_equal(d.x[5], d.x[2]) and np.array_equal(d.x[9], d.x[2]) and in_every_list(cs["identical"], [2, 5, 9])
    d = M.build(cs["zero_row"]).data
    assert not d.x[3].any() and in_every_list(cs["zero_row"], [3])
    c = cs["zero_query"]
    d = M.build(c).data
    assert not d.q[1].any() and d.q[0].any() and M.expect(c).picks[1, 0] == 0                # all cosines 0: position 0 first
    c = cs["near_dup"]
    d = M.build(c).data
    rel = np.linalg.norm(d.x[0].astype(np.float64) - d.x[1]) / np.linalg.norm(d.x[0])
    assert 1e-4 < rel < 1e-2 and not np.array_equal(d.x[0], d.x[1]) and in_every_list(c, range(8))
    d = M.build(cs["pow2"]).data
    assert np.array_equal(d.x[7], d.x[1] * np.float32(4)) and np.array_equal(d.x[8] * np.float32(4), d.x[6]) and in_every_list(cs["pow2"], [1, 6, 7, 8])
    d = M.build(cs["removed"]).data
    assert d.removed and in_every_list(cs["removed"], d.removed)
    if route == "lds":
        one = [c for c in _by("lds") if c.dim == 1]
        assert one and all(c.data == "dim1" for c in one)
        for c in one:
            e = M.expect(c)
            assert e.n_ties >= e.n_decisions // 2                            # every cosine is +-1: nearly every decision is a tie


def test_every_tie_class_is_decided_at_the_top_on_both_routes():
    """The constructed ties must actually be ties BETWEEN THE BEST candidates somewhere, or they test nothing."""
    for route in ("lds", "wave"):
        for name, sel in (("identical", lambda c: c.data == "identical"), ("repeat", lambda c: c.lists == "repeat"),
                          ("pow2", lambda c: c.data == "pow2"), ("zero_query", lambda c: c.data == "zero_query")):
            assert name in M.TIE_CLASSES
            assert sum(M.expect(c).n_ties for c in _by(route) if sel(c)) > 0, (route, name)
    assert "dim1" in M.TIE_CLASSES and set(M.TIE_CLASSES) == {"identical", "repeat", "pow2", "dim1", "zero_query"}
    # the classes are bit-exact by construction: a copy scaled by a power of two has the cosines of its original, bit for bit
    c = next(c for c in M.CASES if c.data == "pow2")
    d = M.build(c).data
    a = M._greedy(d.q[0], d.x[[1, 7, 6, 8, 20]], [True] * 5, 1, 0.5)
    assert a[2][0] == () or set(a[2][0]) in ({0, 1}, {2, 3})
    cos = lambda u, v: M._cos(M._dot(u.astype(np.float64), v.astype(np.float64)), M._dot(u.astype(np.float64), u.astype(np.float64)),
                              M._dot(v.astype(np.float64), v.astype(np.float64)))
    assert cos(d.q[0], d.x[1]) == cos(d.q[0], d.x[7]) and cos(d.x[30], d.x[6]) == cos(d.x[30], d.x[8])


# ---- every decision is settled -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", M.CASES, ids=lambda c: c.id)
def test_every_decision_of_the_case_is_settled(case):
    e = M.expect(case)
    assert not e.unsettled, (case.id, e.unsettled[:5])
    assert e.n_decisions == sum(len(m) for m in e.margins) > 0 or case.lists == "all_absent"
    assert all(m >= M.MARGIN_MIN or m == 0.0 for ms in e.margins for m in ms)


def test_share_of_decisions_left_out_is_zero():
    total = sum(M.expect(c).n_decisions for c in M.CASES)
    ties = sum(M.expect(c).n_ties for c in M.CASES)
    left_out = sum(len(M.expect(c).unsettled) for c in M.CASES)
    low = min(M.expect(c).min_margin for c in M.CASES)
    print(f"\n{len(M.CASES)} cases, {total} decisions: {total - ties} with a margin >= {low:.2e}, {ties} exact ties inside a constructed class, "
          f"{left_out} left out")
    assert left_out == 0 and total > 2000 and low >= M.MARGIN_MIN
    assert M.MARGIN_MIN >= 30 * (2 * (2 * 3072 + 6) * 2.0 ** -53 * 2)        # the bound of the comment in mmr_regimes.py, with its factor 30


# ---- the reference is right ------------------------------------------------------------------------------------------------------------
def test_ref_mmr_worked_examples():
    f = lambda *r: np.array(r, np.float32)
    # q = (1, 0); cosines to q: x0 = (4, 3): 0.8, x1 = (3, 4): 0.6, x2 = (3, -4): 0.6; cos(x1, x0) = 24/25, cos(x2, x0) = 0, cos(x1, x2) = -7/25
    q, x = f(1, 0), f([4, 3], [3, 4], [3, -4])
    all3 = [True] * 3
    # lambda 0.5: x0 first; then x1: 0.3 - 0.5 * 0.96 = -0.18, x2: 0.3 - 0 = 0.3 -> x2; then x1
    picks, margins, ties = M.ref_mmr(q, x, all3, 3, 0.5)
    assert picks == [0, 2, 1] and ties == [False] * 3
    assert abs(margins[0] - 0.2) < 1e-15 and abs(margins[1] - 0.48) < 1e-15 and margins[2] == np.inf
    # lambda 1: plain ranking by cosine, and x1 | x2 tie exactly at 0.6: the lower position first
    picks, margins, ties = M.ref_mmr(q, x, all3, 3, 1.0)
    assert picks == [0, 1, 2] and ties == [False, True, False] and margins[1] == 0.0
    # lambda 0: the least redundant candidate second (x2: -0 against x1: -0.96), whatever its relevance
    assert M.ref_mmr(q, x, all3, 2, 0.0)[0] == [0, 2]
    assert M.ref_mmr(f(0, 1), x, all3, 2, 0.0)[0] == [1, 2]                   # first x1 (0.8); then x0: -0.96, x2: +0.28 -> x2
    # absent candidates are skipped and do not count; the output is padded to k
    assert M.ref_mmr(q, x, [False, True, True], 5, 0.5)[0] == [1, 2, -1, -1, -1]
    assert M.ref_mmr(q, x, [False] * 3, 2, 0.5) == ([-1, -1], [], [])
    # a zero row and a zero query: every quotient that is not finite counts as 0
    picks, margins, ties = M.ref_mmr(f(0, 0), x, all3, 3, 0.5)
    assert picks[0] == 0 and ties[0] and margins[0] == 0.0
    picks, _, _ = M.ref_mmr(q, f([-1, 0], [0, 0], [-1, 1]), all3, 3, 0.5)     # cosines -1, 0 (the zero row), -0.707
    assert picks[0] == 1


def test_ref_mmr_with_lambda_one_ranks_by_cosine():
    rng = np.random.default_rng(3)
    x = rng.standard_normal((30, 17)).astype(np.float32)
    q = rng.standard_normal(17).astype(np.float32)
    cos = (x.astype(np.float64) @ q) / (np.linalg.norm(x.astype(np.float64), axis=1) * np.linalg.norm(q.astype(np.float64)))
    assert M.ref_mmr(q, x, [True] * 30, 30, 1.0)[0] == np.argsort(-cos, kind="stable").tolist()


def test_ref_mmr_skips_absent_candidates_like_a_shorter_list():
    rng = np.random.default_rng(4)
    x = rng.standard_normal((20, 33)).astype(np.float32)
    q = rng.standard_normal(33).astype(np.float32)
    valid = rng.random(20) < 0.6
    live = np.flatnonzero(valid)
    short = M.ref_mmr(q, x[live], [True] * live.size, 25, 0.4)[0]
    full = M.ref_mmr(q, x, valid, 25, 0.4)[0]
    assert full == [int(live[p]) if p >= 0 else -1 for p in short] and full[live.size:] == [-1] * (25 - live.size)


_NO_ABSENT = [c for c in M.CASES if c.data != "removed" and M.valid_mask(c, M.build(c).rows).all()]


def test_the_oracle_comparison_covers_most_of_the_table():
    assert len(_NO_ABSENT) >= len(M.CASES) // 2 and {c.route for c in _NO_ABSENT} == {"lds", "wave"}


@pytest.mark.parametrize("case", _NO_ABSENT, ids=lambda c: c.id)
def test_ref_mmr_equals_the_fp64_oracle(case):
    """oracle.mmr is langchain's numpy code (BLAS dot products in fp64): its sums are ordered differently again, and every decision is settled,
    so the picks are equal.  (The oracle returns min(k, n) picks without padding.)"""
    b = M.build(case)
    stored = M.normalised(b.data.x) if case.metric == "cosine" else b.data.x
    want = M.expect(case).picks
    for qi in range(case.distinct):
        got = O.mmr(b.data.q[qi], stored[b.rows[qi]], k=case.k, lambda_mult=case.lam)
        n = min(case.k, case.fetch_k)
        assert got == want[qi, :n].tolist() and (want[qi, n:] == -1).all(), (case.id, qi)


# ---- removed rows ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [c for c in M.CASES if c.data == "removed"], ids=lambda c: c.id)
def test_removed_row_cases_tell_absent_from_a_zero_cosine_candidate(case):
    """A removed row is NaN-poisoned: a kernel that takes it for a candidate computes cosine 0 for it everywhere (the NaN -> 0 rule), so
    its objective is 0 and it is picked as soon as every other candidate's redundancy outweighs its relevance.  The contract says the row
    is absent.  The case is only worth running if the two differ -- for every query of the case, and with settled decisions on both sides."""
    b = M.build(case)
    absent, zero = M.expect(case), M.expect(case, removed_as_zero_row=True)
    assert not absent.unsettled and not zero.unsettled
    for qi in range(case.distinct):
        pos = int(np.flatnonzero(b.rows[qi] == b.data.removed[0])[0])
        assert pos not in absent.picks[qi] and pos in zero.picks[qi], (case.id, qi)
        assert not np.array_equal(absent.picks[qi], zero.picks[qi])
