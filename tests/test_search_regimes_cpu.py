"""The search dispatcher's re-run classes, guarded without a GPU.

tests/search_regimes.py restates which branch of `rmu_index_search` answers a block and which of the three device-predicated
launches re-runs its flagged queries (ragmeup_amd/csrc/rmu_api.hip); tests/test_search_regimes_gpu.py holds every class from both
sides of each boundary.  Here:
  * every constant the helper restates is read back out of rmu_api.hip / rmu_common.h and must equal it -- a rework that moves a
    threshold fails here, naming it, and the GPU boundary cases have to follow;
  * for every block size 1 .. 8192 the classes partition the flagged counts 1 .. nb -- on the restated table AND on the (lo, hi)
    pairs of c1 / c2 / c3 parsed from the source and evaluated in Python: every count is answered by exactly one launch, planned for
    at least that many queries or for the whole block;
  * CASES reaches every class and every class boundary from both sides;
  * the verdict of every query of the cases over small corpora (at most CPU_MAX_ROWS rows, at most 1024 queries) is re-derived:
    background margins >= 5 EPS, flagged queries certain-fail, flagged positions at both ends and in one adjacent pair; a seeded sample
    of each case is re-computed by brute force over the FINAL corpus (clusters and deletions included) with eps() of
    tests/test_screen_bound_cpu.py.  Left to the GPU file's control search (nothing may flag among the background alone): the
    270 000-row deep-k cases, the 8192-query cases and the two multi-block requests -- their margins come from the same builder,
    but are not re-computed here because of their size.
"""
import functools
import os
import re

import numpy as np
import pytest

from oracle import oracle as O
from tests import search_regimes as R
from tests.test_screen_bound_cpu import eps as eps_ref, eps_l2 as eps_l2_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_STALE = "the search dispatch moved: update tests/search_regimes.py and its GPU boundary cases (tests/test_search_regimes_gpu.py)"


def _read(rel):
    with open(os.path.join(ROOT, rel), encoding="utf-8") as f:
        return re.sub(r"\s+", " ", f.read())


def _api():
    return _read("ragmeup_amd/csrc/rmu_api.hip")


def _search_body():
    src = _api()
    i = src.index('extern "C" int rmu_index_search(')
    return src[i:src.index("// Exact top-k over the rows one ascending list names", i)]


def _common():
    return _read("ragmeup_amd/csrc/rmu_common.h")


_PAYS = (r"const bool screen_pays = nb >= (\d+) \|\| idx->n >= (\d+) \|\| \(nb > (\d+) && idx->n >= (\d+)\) \|\| min_nq_set \|\| "
         r"\(k > (\d+) && idx->n >= (\d+)\);")
_KP_DEEP = r"const int kp = k \+ \(k / (\d+) > (\d+) \? k / (\d+) : (\d+)\); return kp < RMU_KS_CAP_DEEP - (\d+) \? kp : RMU_KS_CAP_DEEP - (\d+);"

# name -> (where, pattern, group, restated value)
SOURCE_CONSTANTS = {
    "kMaxQueriesPerLaunch": (_api, r"static const int64_t kMaxQueriesPerLaunch = (\d+);", 1, R.MAX_QUERIES_PER_LAUNCH),
    "one_class: nb <= 32": (_search_body, r"const bool one_class = nb <= (\d+);", 1, R.ONE_CLASS_MAX_NB),
    "small_n: nb < 32": (_search_body, r"small_n = \(int\)\(nb < (\d+) \? nb : (\d+)\)", 1, R.SMALL_N),
    "small_n: 32": (_search_body, r"small_n = \(int\)\(nb < (\d+) \? nb : (\d+)\)", 2, R.SMALL_N),
    "mid_n: nb / 8": (_search_body, r"mid_n = one_class \? 0 : \(int\)\(nb / (\d+)\)", 1, R.MID_DIV),
    "kScreenKp": (_api, r"static const int kScreenKp = (\d+);", 1, R.SCREEN_KP),
    "screen_kp: k <= 24": (_api, r"if \(k <= (\d+)\) return kScreenKp;", 1, R.KP_STEP1),
    "screen_kp: k <= 32": (_api, r"return kScreenKp; if \(k <= (\d+)\) return (\d+);", 1, R.KP_STEP2),
    "screen_kp: 40": (_api, r"return kScreenKp; if \(k <= (\d+)\) return (\d+);", 2, R.KP_AT_STEP2),
    "screen_kp: k / 5": (_api, _KP_DEEP, 1, R.KP_DEEP_DIV),
    "screen_kp: k / 5 (taken)": (_api, _KP_DEEP, 3, R.KP_DEEP_DIV),
    "screen_kp: at least 8": (_api, _KP_DEEP, 2, R.KP_DEEP_MIN),
    "screen_kp: at least 8 (taken)": (_api, _KP_DEEP, 4, R.KP_DEEP_MIN),
    "screen_kp: cap - 8": (_api, _KP_DEEP, 5, R.KS_CAP_DEEP - R.KP_DEEP_MAX),
    "screen_kp: cap - 8 (taken)": (_api, _KP_DEEP, 6, R.KS_CAP_DEEP - R.KP_DEEP_MAX),
    "kScreenMaxK": (_api, r"static const int kScreenMaxK = (\d+);", 1, R.SCREEN_MAX_K),
    "screen_pays: nb >= 128": (_api, _PAYS, 1, R.PAYS_NB),
    "screen_pays: n >= 3000000": (_api, _PAYS, 2, R.PAYS_N),
    "screen_pays: nb > 64": (_api, _PAYS, 3, R.PAYS_MID_NB),
    "screen_pays: n >= 1000000": (_api, _PAYS, 4, R.PAYS_MID_N),
    "screen_pays: k > 32": (_api, _PAYS, 5, R.DEEP_K),
    "screen_pays: n >= 262144": (_api, _PAYS, 6, R.DEEP_N),
    "deep_applies: k > 32": (_api, r"return !off && k > (\d+) && idx->n >= (\d+);", 1, R.DEEP_K),
    "deep_applies: n >= 262144": (_api, r"return !off && k > (\d+) && idx->n >= (\d+);", 2, R.DEEP_N),
    "geom: dim == 384": (_api, r"const bool geom = idx->dim == (\d+) && \(idx->metric == RMU_METRIC_L2SQ \? idx->nrm != nullptr : idx->dpad == (\d+)\);", 1, R.SCREEN_DIM),
    "geom: dpad == 384": (_api, r"const bool geom = idx->dim == (\d+) && \(idx->metric == RMU_METRIC_L2SQ \? idx->nrm != nullptr : idx->dpad == (\d+)\);", 2, R.SCREEN_DIM),
    "xnorm_max < 500.f": (_api, r"idx->xnorm_max > 0\.f && idx->xnorm_max < (\d+)\.f;", 1, int(R.XNORM_CAP)),
    "RMU_KS_CAP": (_common, r"#define RMU_KS_CAP (\d+) ", 1, R.KS_CAP),
    "RMU_KS_CAP_DEEP": (_common, r"#define RMU_KS_CAP_DEEP (\d+) ", 1, R.KS_CAP_DEEP),
}

# structural facts the restated tables rely on (no number to compare: the pattern must simply be there)
SOURCE_SHAPES = {
    "screen_applies: every condition": (_api,
        r"return idx->split && idx->screen_enabled && geom && nb >= screen_min_nq && screen_pays && k <= kScreenMaxK && idx->n > 0 && "
        r"idx->xnorm_max > 0\.f && idx->xnorm_max < "),
    "a minimum batch that was set makes the screen pay": (_api, r"const bool min_nq_set = env_set \|\| idx->screen_min_nq > 0;"),
    "branch order: screen, deep ladder, exact": (_search_body,
        r"const bool screened = screen_applies\(idx, nb, k\); if \(screened\) rc = search_block_screened\(b\); "
        r"else if \(deep_applies\(idx, k\)\) rc = search_block_deep\(b\); else rc = search_block_exact\(b\); if \(rc\) return rc;"),
    "the block loop": (_search_body,
        r"for \(int64_t q0 = 0; q0 < nq; q0 \+= kMaxQueriesPerLaunch\) \{ const int64_t nb = \(nq - q0\) < kMaxQueriesPerLaunch \? \(nq - q0\) : kMaxQueriesPerLaunch;"),
    "outputs of block q0 start at q0 * k": (_search_body, r"float\* d_s = out_scores \+ q0 \* k; int64_t\* d_r = out_rows \+ q0 \* k;"),
    # (anchored on the identifiers only: the launch a predicate belongs to, the query count it is planned for, gathered list or in place)
    "small launch: planned for small_n, gathered, scattered": (_search_body,
        r"lim_small > 0 && \(rc = plan_exact\(b, [^;]*\bsmall_n, &c1, &L1\).*if \(lim_small > 0 && \(rc = run_exact\(b, L1, d_s, d_r, [^,;]*\bfb_i\b"),
    "mid launch: planned for mid_n, gathered, scattered": (_search_body,
        r"mid_n > small_n && \(rc = plan_exact\(b, [^;]*\bmid_n, &c2, &L2\).*if \(mid_n > small_n && \(rc = run_exact\(b, L2, d_s, d_r, [^,;]*\bfb_i\b"),
    "whole launch: planned for nb, in place": (_search_body,
        r"\(rc = plan_exact\(b, qdev, nb, &c3, &L3\)\).*[^{] if \(\(rc = run_exact\(b, L3, d_s, d_r, nullptr,"),
    "the re-run count is summed over the drained blocks": (_search_body,
        r"if \(drained\) rerun_total \+= [^;]*hflag;.*screened = any_screened \? \(rerun_total \? -rerun_total : 1\) : 0;"),
}


@pytest.mark.parametrize("name", list(SOURCE_CONSTANTS))
def test_constant_matches_the_source(name):
    where, pat, group, want = SOURCE_CONSTANTS[name]
    m = re.search(pat, where())
    assert m, f"{name}: pattern not found in the source -- {_STALE}"
    assert int(m.group(group)) == want, f"{name}: the source says {m.group(group)}, tests/search_regimes.py says {want} -- {_STALE}"


@pytest.mark.parametrize("name", list(SOURCE_SHAPES))
def test_dispatch_shape_matches_the_source(name):
    where, pat = SOURCE_SHAPES[name]
    assert re.search(pat, where()), f"{name}: not found in the source -- {_STALE}"


def test_screen_kp_steps():
    assert [R.screen_kp(k) for k in (1, 10, 24, 25, 28, 32, 33, 40, 41, 45, 100, 104)] == [32, 32, 32, 40, 40, 40, 41, 48, 49, 54, 120, 120]
    assert all(R.screen_kp(k) >= k + 8 for k in range(1, R.SCREEN_MAX_K + 1))
    assert max(R.screen_kp(k) for k in range(1, R.KP_STEP2 + 1)) + 8 == R.KS_CAP and R.screen_kp(R.SCREEN_MAX_K) + 8 == R.KS_CAP_DEEP


def test_path_restates_the_branch():
    assert R.path(20_000, 1024, 10, 384) == "screen" and R.path(20_000, 128, 10, 384) == "screen"
    assert R.path(20_000, 127, 10, 384) == "exact" and R.path(20_000, 127, 10, 384, min_nq=1) == "screen"
    assert R.path(20_000, 7, 10, 384, min_nq=8) == "exact"
    assert R.path(1_000_000, 65, 10, 384) == "screen" and R.path(1_000_000, 64, 10, 384) == "exact" and R.path(3_000_000, 1, 10, 384) == "screen"
    assert R.path(262_144, 1, 33, 384) == "screen" and R.path(262_143, 1, 33, 384) == "exact" and R.path(262_144, 1, 32, 384) == "exact"
    assert R.path(262_144, 1, 104, 384) == "screen" and R.path(262_144, 1024, 105, 384) == "deep_ladder"
    assert R.path(262_144, 1024, 40, 384, screening=False) == "deep_ladder" and R.path(20_000, 1024, 40, 384, screening=False) == "exact"
    assert R.path(20_000, 1024, 10, 256) == "exact" and R.path(20_000, 1024, 10, 384, xnorm_max=500.0) == "exact"
    assert R.path(0, 1024, 10, 384) == "exact"
    assert R.blocks(1) == [(0, 1)] and R.blocks(8192) == [(0, 8192)] and R.blocks(8193) == [(0, 8192), (8192, 1)]
    assert R.blocks(8192 * 2 + 300) == [(0, 8192), (8192, 8192), (16384, 300)]


# ---- c1 / c2 / c3 as the source writes them, evaluated in Python -----------------------------------------------------------------
def _py(expr: str) -> str:
    """A C integer expression of the kind rmu_index_search uses (casts, ?:, ||, &&, /) as a Python one."""
    e = expr.strip()
    e = re.sub(r"\((?:int|int64_t|size_t)\)", "", e)
    depth, q = 0, -1
    for i, ch in enumerate(e):                      # the first top-level '?' splits a conditional; its ':' is the matching top-level one
        depth += ch == "("
        depth -= ch == ")"
        if ch == "?" and depth == 0:
            q = i
            break
    if q >= 0:
        depth, nest = 0, 0
        for j in range(q + 1, len(e)):
            ch = e[j]
            depth += ch == "("
            depth -= ch == ")"
            if depth == 0 and ch == "?":
                nest += 1
            if depth == 0 and ch == ":":
                if nest == 0:
                    return f"(({_py(e[q + 1:j])}) if ({_py(e[:q])}) else ({_py(e[j + 1:])}))"
                nest -= 1
        raise ValueError(expr)
    out, i = "", 0
    while i < len(e):
        if e[i] == "(":
            depth, j = 1, i + 1
            while depth:
                depth += e[j] == "("
                depth -= e[j] == ")"
                j += 1
            out += "(" + _py(e[i + 1:j - 1]) + ")"
            i = j
        else:
            j = i
            while j < len(e) and e[j] != "(":
                j += 1
            out += e[i:j].replace("||", " or ").replace("&&", " and ").replace("/", "//")
            i = j
    return out


def _source_launches():
    """[(class, lo, hi, planned, clamp, guard)] as Python expressions over nb, parsed from the `screened` branch."""
    body = _search_body()
    defs = {}
    m = re.search(r"const bool one_class = ([^;]+);", body)
    defs["one_class"] = _py(m.group(1))
    m = re.search(r"const int small_n = (.+?), mid_n = ([^;]+);", body)
    defs["small_n"], defs["mid_n"] = _py(m.group(1)), _py(m.group(2))
    m = re.search(r"const int lim_small = ([^;]+);", body)
    defs["lim_small"] = _py(m.group(1))
    m = re.search(r"const RmuCond c1\{cnt, (.+?), (.+?), (\d)\}, c2\{cnt, (.+?), (.+?), (\d)\}, c3\{cnt, (.+?), (0x7fffffff), (\d)\};", body)
    assert m, f"c1 / c2 / c3 -- {_STALE}"
    g = [m.group(i) for i in range(1, 10)]
    return defs, [("small", _py(g[0]), _py(g[1]), "small_n", int(g[2]), "lim_small > 0"),
                  ("mid", _py(g[3]), _py(g[4]), "mid_n", int(g[5]), "mid_n > small_n"),
                  ("whole", _py(g[6]), _py(g[7]), "nb", int(g[8]), "True")]


@functools.lru_cache(maxsize=None)
def _code(expr):
    return compile(expr, "<rmu_api.hip>", "eval")


def _source_intervals(nb, defs, launches):
    env = {"nb": nb}
    for name in ("one_class", "small_n", "mid_n", "lim_small"):
        env[name] = eval(_code(defs[name]), {}, env)
    out = []
    for cls, lo, hi, planned, clamp, guard in launches:
        if eval(_code(guard), {}, env):
            out.append((cls, int(eval(_code(lo), {}, env)), int(eval(_code(hi), {}, env)), int(eval(_code(planned), {}, env)), clamp))
    return out


def test_translated_expressions():
    assert eval(_py("(int)(nb < 32 ? nb : 32)"), {}, {"nb": 7}) == 7 and eval(_py("(int)(nb < 32 ? nb : 32)"), {}, {"nb": 70}) == 32
    assert eval(_py("one_class ? 0 : (mid_n > small_n ? small_n : mid_n)"), {}, {"one_class": False, "mid_n": 4, "small_n": 32}) == 4
    assert eval(_py("(a > 0 || b > c ? b : 0) + 1"), {}, {"a": 0, "b": 5, "c": 9}) == 1
    assert eval(_py("one_class ? 0 : (int)(nb / 8)"), {}, {"one_class": False, "nb": 263}) == 32


def test_rerun_classes_partition_every_count_in_source_and_restated():
    defs, launches = _source_launches()
    for nb in range(1, R.MAX_QUERIES_PER_LAUNCH + 1):
        iv = sorted((lo, min(hi, nb), cls, planned, clamp) for cls, lo, hi, planned, clamp in _source_intervals(nb, defs, launches) if lo <= min(hi, nb))
        # the launches that can run tile 1 .. nb: no count unanswered (an off-by-one in lo / hi), none answered twice
        assert iv[0][0] == 1 and iv[-1][1] == nb, (nb, iv)
        for a, b in zip(iv, iv[1:]):
            assert b[0] == a[1] + 1, (nb, iv)
        for lo, hi, cls, planned, clamp in iv:
            assert planned >= hi or planned == nb, (nb, iv)                # room for every query it may be handed
            assert clamp == (0 if cls == "whole" else 1), (nb, iv)        # a gathered launch scans only the flagged ones
            want = "whole_one_class" if nb <= R.ONE_CLASS_MAX_NB else cls
            for c in {lo, hi, (lo + hi) // 2}:
                assert R.rerun_class(nb, c) == (want, planned), (nb, c, iv)
        # ... and the restated table by itself: at every count for the narrow blocks, at every breakpoint for all of them
        counts = range(1, nb + 1) if nb <= 600 else sorted({1, 2, R.SMALL_N - 1, R.SMALL_N, R.SMALL_N + 1, nb // R.MID_DIV - 1, nb // R.MID_DIV,
                                                             nb // R.MID_DIV + 1, nb - 1, nb})
        for c in counts:
            cls, planned = R.rerun_class(nb, c)
            hit = [v for v in iv if v[0] <= c <= v[1]]
            assert len(hit) == 1 and planned == hit[0][3] and (planned >= c or planned == nb), (nb, c, iv)
            assert cls == ("whole_one_class" if nb <= R.ONE_CLASS_MAX_NB else hit[0][2]), (nb, c, iv)
        assert R.rerun_class(nb, 0) == ("none", 0)


# ---- the cases ------------------------------------------------------------------------------------------------------------------
ISSUE_TABLE = {1: (0, 1), 7: (1, 7), 32: (0, 1, 32), 33: (0, 1, 4, 5, 33), 130: (16, 17), 256: (32, 33), 263: (32, 33), 264: (32, 33, 34),
               300: (1, 37, 38), 1024: (0, 1, 31, 32, 33, 127, 128, 129, 1024), 8192: (1024, 1025)}


def _plain(c):
    """a case of the inner-product table: one flagged query has a graded cluster; from two on there is an overflow query, from three on
    graded clusters too"""
    return (c.metric == "ip" and c.k == 10 and not (c.tomb or c.row_base or c.copies) and c.overflow == (c.count >= 2)
            and c.graded == (1 if c.count == 1 else min(4, max(0, c.count - 2))))


def test_cases_hold_the_required_table():
    have = {(c.nb, c.count) for c in R.CASES if _plain(c)}
    missing = [(nb, c) for nb, cs in ISSUE_TABLE.items() for c in cs if (nb, c) not in have]
    assert not missing, missing


def test_cases_reach_every_class_and_every_boundary_from_both_sides():
    one = [c for c in R.CASES if len(c.c) == 1]
    assert {c.classes[0] for c in one} == {"none", "whole_one_class", "small", "mid", "whole"}
    have = {(c.nb, c.count) for c in one if _plain(c)}

    def both_sides(nb, c, below, above):
        return (nb, c) in have and (nb, c + 1) in have and R.rerun_class(nb, c)[0] == below and R.rerun_class(nb, c + 1)[0] == above

    nbs = sorted({nb for nb, _ in have})
    # nb / 8 where no mid launch exists (33 <= nb <= 263): small | whole -- incl. nb / 8 = 32, the widest such block
    assert any(both_sides(nb, nb // 8, "small", "whole") for nb in nbs if 33 <= nb < 256)
    assert both_sides(263, 32, "small", "whole") and both_sides(256, 32, "small", "whole")
    # nb / 8 where it does (nb >= 264): mid | whole -- incl. the narrowest such block, whose mid class is the single count 33
    assert both_sides(264, 33, "mid", "whole") and both_sides(1024, 128, "mid", "whole") and both_sides(8192, 1024, "mid", "whole")
    # 32: small | mid
    assert both_sides(264, 32, "small", "mid") and both_sides(1024, 32, "small", "mid")
    # one_class: the widest block of it and the first one past it, each with one flagged query and with all flagged
    assert {(32, 1), (32, 32), (33, 1), (33, 33)} <= have
    # two query tiles, the second one partial
    assert both_sides(300, 37, "mid", "whole") and (300, 1) in have
    # the other axes: each a small-, a mid- and a whole-class count at 1024 queries and one flagged query of seven
    for pred in (lambda c: c.metric == "l2", lambda c: c.metric == "cosine", lambda c: c.k == 28, lambda c: c.k == 100, lambda c: c.k == 40,
                 lambda c: c.row_base == 1_000_000_007, lambda c: c.tomb):
        got = {(c.nb, c.classes[0]) for c in one if pred(c)}
        assert {(1024, "small"), (1024, "mid"), (1024, "whole"), (7, "whole_one_class")} <= got, got
    assert all(c.n >= R.DEEP_N for c in one if c.k > 32) and R.screen_kp(28) == 40
    assert any(c.copies == 136 and c.k == 100 for c in one) and R.screen_kp(100) + 8 == R.KS_CAP_DEEP
    # a query that is exactly tied keeps a right answer when nobody re-runs it; every case on either side of a boundary therefore holds
    # queries whose un-re-run answer is wrong (`have` is built from such cases only: _plain), and so do the multi-block requests
    assert all(c.overflow and c.graded == 4 for c in R.BLOCK_CASES)
    assert any(not c.overflow and not c.graded and c.count > 1 for c in one if c.metric == "ip" and c.k == 10)      # ... and ties alone stay covered
    assert [c.classes for c in R.BLOCK_CASES] == [["mid", "whole_one_class"], ["small", "whole"]]
    assert [(c.nb, c.c) for c in R.BLOCK_CASES] == [(8192 + 5, (40, 1)), (8192 + 300, (3, 38))] and 38 == 300 // 8 + 1


def test_case_ids_name_their_class_and_every_block_is_screened():
    ids = [c.id for c in R.CASES + R.BLOCK_CASES]
    assert len(ids) == len(set(ids))
    for c in R.CASES + R.BLOCK_CASES:
        assert len(c.c) == len(R.blocks(c.nb)) and all(0 <= cb <= nbb for (_, nbb), cb in zip(R.blocks(c.nb), c.c)), c.id
        assert all(R.path(c.n, nbb, c.k, 384, c.metric, min_nq=c.min_batch) == "screen" for _, nbb in R.blocks(c.nb)), c.id
        if len(c.c) == 1:
            assert f"-nb{c.nb}-c{c.count}-{c.classes[0]}" in c.id, c.id
        assert not c.overflow or (c.metric == "ip" and c.count >= 2)        # (cosine would normalise the overflow away)


# ---- the helper's own arithmetic --------------------------------------------------------------------------------------------------
def test_eps_and_top_lists_agree_with_their_originals():
    rng = np.random.default_rng(4)
    x = (rng.standard_normal((700, 384)) * rng.uniform(0.3, 2.0, (700, 1))).astype(np.float32)
    q = (x[:9] + 0.1 * rng.standard_normal((9, 384))).astype(np.float32)
    dx, xn = R.corpus_maxima(x)
    assert np.allclose(R.eps_numpy(dx, xn, q), eps_ref(x, q), rtol=1e-12) and np.allclose(R.eps_numpy(dx, xn, q, l2=True), eps_l2_ref(x, q), rtol=1e-12)
    xd = np.concatenate([x, np.repeat(x[3:4], 20, axis=0)])
    alive = np.ones(720, bool)
    alive[[3, 701, 705]] = False
    for metric, om in (("ip", O.METRIC_IP), ("cosine", O.METRIC_COSINE), ("l2", O.METRIC_L2SQ)):
        s, r = R.oracle_topk(q, xd, 12, metric, alive=alive, budget=720 * 4)
        s0, r0 = O.flat_search(q, xd, 12, om, alive=alive)
        assert np.array_equal(np.sort(r, axis=1), np.sort(r0, axis=1)) and np.allclose(s, s0, rtol=0, atol=1e-12)
        ts, tr = R._top_lists(q, x, 12, "l2" if metric == "l2" else "ip")
        s1, r1 = O.flat_search(q, x, 12, O.METRIC_L2SQ if metric == "l2" else O.METRIC_IP)
        assert np.array_equal(tr, r1) and np.allclose(ts, s1, rtol=0, atol=1e-9)
    rep = np.arange(720)
    rep[700:] = 3                                   # exact copies take their original's score: ties come out in ascending row order
    s, r = R.oracle_topk(xd[700:701], xd, 12, "ip", rep=rep)
    assert np.array_equal(r[0], np.concatenate([[3], 700 + np.arange(11)])) and (s[0] == s[0, 0]).all()
    s, r = R.oracle_topk(q[:2], x[:5], 8)
    assert (r[:, 5:] == -1).all() and np.isneginf(s[:, 5:]).all() and (np.sort(r[:, :5], axis=1) == np.arange(5)).all()


# ---- the verdicts, re-derived ---------------------------------------------------------------------------------------------------------
CPU_CASES = [c for c in R.CASES if c.n <= R.CPU_MAX_ROWS and c.nb <= 1024]


def test_which_cases_are_left_to_the_gpu_control_search():
    left = [c for c in R.CASES if c not in CPU_CASES]
    assert all(c.n >= R.DEEP_N or c.nb == 8192 for c in left) and len(CPU_CASES) >= 50 and len(BRUTE_CASES) >= 10


# ... of these, the ones whose sample is re-computed by brute force over the final corpus: per axis the mid-class count at 1024 queries, plus
# a seven-query block, the all-flagged 1024 (shared, perturbed clusters) and a case with an fp16 overflow and graded clusters
BRUTE_CASES = [c for c in CPU_CASES if (c.nb, c.count) in ((1024, 40), (1024, 33), (1024, 1024), (130, 17)) or c.id == "ip-nb7-c1-whole_one_class"]


@pytest.mark.parametrize("case", CPU_CASES, ids=[c.id for c in CPU_CASES])
def test_verdicts_of_the_case(case):
    b = R.build(case)
    nb, k, kp = case.nb, case.k, case.kp
    assert b.q.shape == (nb, 384) and np.isfinite(b.q).all() and b.flagged.size == case.count == (b.kinds != "b").sum()
    assert (b.kinds[b.flagged] != "b").all() and (np.diff(b.flagged) > 0).all()
    bg, tie, grd = np.nonzero(b.kinds == "b")[0], np.nonzero(b.kinds == "t")[0], np.nonzero(b.kinds == "g")[0]
    assert (b.margins[bg] >= R.MARGIN_EPS).all() and (b.margins[tie] >= R.MARGIN_EPS).all() and (b.margins[grd] >= R.MARGIN_EPS).all()
    assert grd.size == case.graded and set(b.graded_rows) == set(grd.tolist())
    for p, rows in b.graded_rows.items():
        # one fp16 image (one approximate score: certain-fail), exact scores growing with the row id in steps the tie rule resolves; the K'
        # lowest ids -- what the screen keeps of equal scores -- hold at most two of the true top k, the rest lies more than the tie rule's 1e-6 above all of them
        assert (R._image(b.x[rows]) == R._image(b.x[rows[:1]])).all() and (np.diff(rows) > 0).all() and rows.size >= kp + 9
        sc = b.x[rows].astype(np.float64) @ b.q[p].astype(np.float64)
        assert (np.diff(sc[1:]) > 2e-6).all()
        top = rows[np.lexsort((rows, -sc))][:k]
        kept = rows[:kp]
        assert np.isin(top, kept).sum() <= 2 and sc[np.isin(rows, top) & ~np.isin(rows, kept)].min() - sc[:kp].max() > 2e-6
    assert (b.kinds == "o").sum() == (1 if case.overflow else 0)
    for i in np.nonzero(b.kinds == "o")[0]:
        assert np.abs(b.q[i]).max() * 64.0 > 65504.0
    # positions: the last query from one flagged on, the first from two, an adjacent pair from four (or every query)
    f = set(b.flagged.tolist())
    assert case.count < 1 or nb - 1 in f
    assert case.count < 2 or 0 in f
    assert case.count < 4 or any(p + 1 in f for p in f)
    assert b.spare.shape[0] == R.N_SPARE
    # own clusters: no two tie queries share an answer while there are at most MAX_CLUSTERS of them
    assert set(b.expect) == set(tie.tolist()) and all(v.shape == (k,) and (np.diff(v) > 0).all() for v in b.expect.values())
    if tie.size <= R.MAX_CLUSTERS:
        assert len({tuple(v) for v in b.expect.values()}) == tie.size
    alive = b.alive
    assert not alive[b.dead].any() and (len(b.dead) > 0) == (case.tomb and tie.size > 0)
    if case not in BRUTE_CASES:
        return
    # brute force over the final corpus, for a seeded sample: EPS is eps() of tests/test_screen_bound_cpu.py over the live rows
    rng = np.random.default_rng(nb * 1000 + case.count)
    pick = np.concatenate([rng.permutation(bg)[:16], rng.permutation(tie)[:4], grd[:2]]).astype(np.int64)
    xs, qs = b.x[alive], b.q[pick]
    if case.metric == "cosine":
        xs, qs = R._unit32(xs), R._unit32(qs)
    e = eps_l2_ref(xs, qs) if case.metric == "l2" else eps_ref(xs, qs)
    half = 0.5 if case.metric == "l2" else 1.0
    s, r = R.oracle_topk(b.q[pick], b.x, kp + 10, case.metric, alive=alive, rep=b.rep)      # (a cluster has at most K' + 9 live rows)
    for j, p in enumerate(pick):
        if b.kinds[p] == "b":
            m = half * (s[j, k - 1] - s[j, kp - 1]) / e[j]
            assert m >= R.MARGIN_EPS and abs(m - b.margins[p]) <= 1e-4 * m, (p, m, b.margins[p])
        else:
            # the K' best are copies of one row (equal scores, ascending ids), all of this query's own
            # cluster, and the first row that is not a copy lies >= 5 EPS below
            if b.kinds[p] == "g":
                same = (R._image(b.x[r[j]]) == R._image(b.x[r[j, :1]])).all(axis=1)
                assert same[:kp].all() and not same.all() and np.array_equal(np.sort(r[j, same]), b.graded_rows[int(p)])
                m = (s[j, same].min() - s[j, ~same][0]) / e[j]
                assert m >= R.MARGIN_EPS and abs(m - b.margins[p]) <= 1e-4 * m, (p, m, b.margins[p])
                continue
            same = (b.x[r[j]] == b.x[r[j, 0]]).all(axis=1)
            assert same[:kp].all() and not same.all() and s[j, 0] == s[j, kp - 1] and (np.diff(r[j, :kp]) > 0).all()
            cluster = np.sort(r[j, same])
            assert np.array_equal(b.expect[int(p)], cluster[:k]) and (cluster[1:] >= case.n).all()
            m = half * (s[j, 0] - s[j, ~same][0]) / e[j]
            assert m >= R.MARGIN_EPS and abs(m - b.margins[p]) <= 1e-4 * m, (p, m, b.margins[p])


@pytest.mark.parametrize("cid", ["ip-nb130-c17-whole", "k28-nb7-c1-whole_one_class", "tomb-nb7-c1-whole_one_class", "ip-nb33-c5-whole"])
def test_emulated_screen_flags_exactly_the_flagged_queries(cid):
    """The numpy emulation of the screening arithmetic (tests/test_screen_bound_cpu.py) with the sufficiency test of k_rescore, at the
    largest eps the device may use (1.05 EPS): the queries it fails are the case's flagged queries, no other."""
    from tests.test_screen_bound_cpu import screen_scores
    case = next(c for c in R.CASES if c.id == cid)
    b = R.build(case)
    alive = b.alive
    with np.errstate(all="ignore"):                     # (the overflow query: fp16(64 q) = inf, its scores are NaN, its eps is not finite)
        st = screen_scores(b.x, b.q).astype(np.float64)
        e = 1.05 * eps_ref(b.x[alive], b.q)
    st[:, ~alive] = -np.inf
    st[np.isnan(st)] = -np.inf
    top = -np.sort(-st, axis=1)[:, :case.kp]
    ok = np.isfinite(e) & (top[:, case.kp - 1] < top[:, case.k - 1] - 2.0 * e)
    assert np.array_equal(np.nonzero(~ok)[0], b.flagged)
    for p, rows in b.graded_rows.items():               # a graded cluster is ONE approximate score
        assert (st[p, rows] == st[p, rows[0]]).all()
