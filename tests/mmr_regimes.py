"""The greedy MMR selection (k_mmr_lds and k_mmr in ragmeup_amd/csrc/rmu_api.hip, behind launch_mmr) restated on the host: the dispatch
(`route`), an exact reference (`ref_mmr`), the rule that says when a greedy decision is far enough from a tie to be compared by equality,
builders of candidate lists and of rows, and the table of cases that holds both kernels from both sides of both dispatch thresholds.

A plain helper module, not a fixture: tests/test_mmr_regimes_cpu.py reads every constant below back out of the source, checks that CASES
reaches every route, remainder, list class and data class, and proves that EVERY decision of EVERY case is settled;
tests/test_mmr_regimes_gpu.py runs CASES on the device, and tests/mmr_variant_driver.py runs them once more in a process whose selections
all go through k_mmr (RMU_TUNING=1 RMU_MMR_LDS=0).

The rule (include/rmu.h, rmu_index_mmr): first pick = argmax cos(q, x); then repeatedly argmax lambda * cos(q, x) - (1 - lambda) * max cos(x,
picked); the lowest position wins ties; cos = dot / (|a| |b|), a quotient that is not finite counts as 0.  A candidate is ABSENT when its id
is -1, is not a row of the index (>= n_rows), or names a removed row: it is never picked and does not count toward the number of candidates.
"""
from __future__ import annotations

import functools
import hashlib
import math
import os
import zlib
from dataclasses import dataclass, field

import numpy as np

# ---- constants of launch_mmr / k_mmr / k_mmr_lds (tests/test_mmr_regimes_cpu.py reads them back) --------------------------------------
LDS_MAX_DIM = 384             # dim <= 384: k_mmr_lds may run (the rows of one query fit its LDS area)
LDS_MAX_NQ = 65535            # ... and nq <= 65535 (one workgroup per query)
MAX_FETCH_K = 64              # one lane per candidate
WAVE_QUERIES_PER_WG = 4       # k_mmr: one wave per query, four waves per workgroup
LDS_UNROLL = 4                # k_mmr_lds: four interleaved fma chains over the dimensions
TAIL_STRIDE = 64              # both kernels: the -1 fill past the candidates strides by the wave
LDS_BYTES = (64 * 385 + 384) * 4 + (65 * 64 + 1) * 8
F_Q_DEVICE, F_OUT_DEVICE = 1, 2

FILL_POS = np.int32(-77)      # a value no kernel writes: "this slot was not written"


def lds_on_in_this_process() -> bool:
    """RMU_MMR_LDS is read once per process and only counts with RMU_TUNING=1."""
    return not (os.environ.get("RMU_TUNING") == "1" and os.environ.get("RMU_MMR_LDS") is not None and _atoi(os.environ["RMU_MMR_LDS"]) == 0)


def _atoi(s: str) -> int:
    try:
        return int(s.strip() or 0)
    except ValueError:
        return 0                      # (a switch the tests never set to anything but "0")


def route(dim: int, nq: int, lds_on: bool = True) -> str:
    """launch_mmr: "lds" = k_mmr_lds (one workgroup per query), "wave" = k_mmr (one wave per query)."""
    return "lds" if dim <= LDS_MAX_DIM and nq <= LDS_MAX_NQ and lds_on else "wave"


# ---- the exact reference -----------------------------------------------------------------------------------------------------------
def _dot(a: np.ndarray, b: np.ndarray) -> float:
    """a, b: fp64 arrays that hold fp32 values, so every product is exact in fp64 (24 + 24 bits); math.fsum rounds their sum once."""
    return math.fsum((a * b).tolist())


def _cos(d: float, aa: float, bb: float) -> float:
    den = math.sqrt(aa) * math.sqrt(bb)
    if den == 0.0:
        return 0.0                    # 0 / 0 and x / 0: not finite -> 0
    c = d / den
    return c if math.isfinite(c) else 0.0


def _greedy(q, cand, valid, k: int, lam: float):
    q64 = np.asarray(q, dtype=np.float32).astype(np.float64)
    c64 = np.asarray(cand, dtype=np.float32).astype(np.float64)
    remaining = [i for i in range(c64.shape[0]) if valid[i]]
    qq = _dot(q64, q64)
    nn = {i: _dot(c64[i], c64[i]) for i in remaining}
    sim_q = {i: _cos(_dot(q64, c64[i]), qq, nn[i]) for i in remaining}
    red = {i: -math.inf for i in remaining}
    want = min(int(k), len(remaining))
    picks, margins, tied, gaps = [], [], [], []
    for t in range(want):
        obj = {i: sim_q[i] if t == 0 else lam * sim_q[i] - (1.0 - lam) * red[i] for i in remaining}
        best = max(obj.values())
        ties = tuple(i for i in remaining if obj[i] == best)
        lower = [v for v in obj.values() if v < best]
        gap = best - max(lower) if lower else math.inf          # to the best objective that is NOT equal to the winner's
        sel = ties[0]                                            # the lowest position wins
        picks.append(sel)
        margins.append(0.0 if len(ties) > 1 else gap)
        tied.append(ties if len(ties) > 1 else ())
        gaps.append(gap)
        remaining.remove(sel)
        if t + 1 < want:
            for i in remaining:
                red[i] = max(red[i], _cos(_dot(c64[i], c64[sel]), nn[i], nn[sel]))
    return picks + [-1] * (int(k) - want), margins, tied, gaps


def ref_mmr(q, cand, valid, k: int, lam: float):
    """q [dim] fp32, cand [n, dim] fp32 (the row of an absent candidate is never read), valid [n] bool ->
    (picks: k positions in the candidate list, -1 past the candidates; margins: per pick the gap between the best and the runner-up
    objective, 0.0 on an exact tie, inf with one candidate left; tie_flags: per pick whether the best objective was held by more than one
    candidate).  Every dot product is a correctly rounded sum of exact products."""
    picks, margins, tied, _ = _greedy(q, cand, valid, k, lam)
    return picks, margins, [bool(t) for t in tied]


# ---- the settled-decision rule ---------------------------------------------------------------------------------------------------
# A kernel's fp64 dot product of length dim (a chain of fmas, in whatever order) errs by at most about dim * 2^-53 * |a| |b|; the two
# squared norms, the two square roots, the product of the norms and the division add a few roundings each, so a cosine errs by at most
# about (2 * dim + 6) * 2^-53: 6.8e-13 at dim 3072.  An objective is two such terms with weights lambda and 1 - lambda (<= one cosine's
# error in all, plus two roundings of its own, or one with a contracted fma); a comparison involves two objectives and the reference adds
# half an ulp per cosine of its own: the bound stays below 3e-12.  MARGIN_MIN is more than 30 times that.  A decision whose margin is at
# least MARGIN_MIN is therefore taken the same way by k_mmr, by k_mmr_lds and by the reference, whatever their summation orders.
MARGIN_MIN = 1e-10
# ... or it is an EXACT tie inside one of the constructed classes below, where every kernel computes identical bits for the tied candidates
# (the same operations on the same values), so the lowest position wins everywhere:
TIE_CLASSES = (
    "identical",       # two rows with the same bits
    "repeat",          # one row id twice in a list
    "pow2",            # a power-of-two multiple of another row: the scaling is exact through the dot, the square and the square root
    "dim1",            # dim = 1: every cosine is a * b / (|a| |b|) = +-1 exactly
    "zero_query",      # a zero query: every cos(q, x) is 0 / 0 -> 0, so the FIRST pick is position 0 (the issue's "all cosines 0" case)
)


def settled(margin: float, gap: float, ties, label) -> bool:
    """ties: the positions that hold the best objective (empty: one winner); label(position) names a position's tie class member;
    gap: the distance from the winner to the best objective that differs from it, which must be a clear margin as well."""
    if not ties:
        return margin >= MARGIN_MIN
    return margin == 0.0 and len({label(p) for p in ties}) == 1 and gap >= MARGIN_MIN


# ---- cases -----------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    id: str
    metric: str        # "ip" | "cosine" | "l2"
    dim: int
    n_rows: int        # rows of the index (<= 300)
    nq: int
    fetch_k: int
    k: int
    lam: float
    lists: str         # name of the list builder (LIST_BUILDERS)
    data: str          # name of the data builder (DATA_BUILDERS)
    tile: int = 0      # > 0: that many distinct queries (and lists), repeated to nq

    @property
    def route(self) -> str:
        return route(self.dim, self.nq)

    @property
    def distinct(self) -> int:
        return self.tile or self.nq


@dataclass
class Data:
    x: np.ndarray                                  # [n_rows, dim] fp32, as given to rmu_index_add
    q: np.ndarray                                  # [distinct, dim] fp32
    special: list = field(default_factory=list)    # rows every candidate list must hold
    canon: dict = field(default_factory=dict)      # row -> the row it is a copy of (tie classes "identical" and "pow2")
    removed: list = field(default_factory=list)    # rows removed after the add
    zero_q: set = field(default_factory=set)       # queries that are all zero


def _rows(case: Case, rng):
    x = rng.standard_normal((case.n_rows, case.dim)).astype(np.float32)
    q = rng.standard_normal((case.distinct, case.dim)).astype(np.float32)
    return x, q


def _data_random(case, rng):
    return Data(*_rows(case, rng))


def _data_identical(case, rng):
    x, q = _rows(case, rng)
    x[5] = x[2]
    x[9] = x[2]
    x[7] = x[4]
    return Data(x, q, special=[2, 4, 5, 7, 9], canon={5: 2, 9: 2, 7: 4})


def _data_zero_row(case, rng):
    x, q = _rows(case, rng)
    x[3] = 0.0
    return Data(x, q, special=[3])


def _data_zero_query(case, rng):
    x, q = _rows(case, rng)
    q[1] = 0.0
    return Data(x, q, zero_q={1})


def _data_near_dup(case, rng):
    """Overlapping chunks: groups of four rows that differ by 1e-3 noise; the query sits near one group."""
    x, q = _rows(case, rng)
    groups = -(-case.n_rows // 4)
    noise = 1e-3 * rng.standard_normal((case.n_rows, case.dim))
    x = (np.repeat(x[:groups], 4, axis=0)[: case.n_rows].astype(np.float64) + noise).astype(np.float32)
    q = (x[rng.integers(0, case.n_rows, case.distinct)] + 0.5 * q).astype(np.float32)
    return Data(x, q, special=list(range(8)))


def _data_pow2(case, rng):
    x, q = _rows(case, rng)
    x[7] = x[1] * np.float32(4.0)
    x[8] = x[6] * np.float32(0.25)
    return Data(x, q, special=[1, 6, 7, 8], canon={7: 1, 8: 6})


def _data_dim1(case, rng):
    assert case.dim == 1
    x, q = _rows(case, rng)
    x[np.abs(x) < 0.05] = 0.5                      # no zeros: every cosine is +1 or -1
    q[np.abs(q) < 0.05] = -0.5
    return Data(x, q)


def _data_removed(case, rng):
    x, q = _rows(case, rng)
    return Data(x, q, special=[6], removed=[6])


DATA_BUILDERS = {"random": _data_random, "identical": _data_identical, "zero_row": _data_zero_row, "zero_query": _data_zero_query,
                 "near_dup": _data_near_dup, "pow2": _data_pow2, "dim1": _data_dim1, "removed": _data_removed}


def _perm(case, rng, d: Data):
    """Per query fetch_k distinct rows in random order, the data's special rows among them at random positions."""
    sp = list(d.special)[: case.fetch_k]
    other = np.array([r for r in range(case.n_rows) if r not in set(d.special)], np.int64)
    assert other.size + len(sp) >= case.fetch_k, case.id
    out = np.empty((case.distinct, case.fetch_k), np.int64)
    for i in range(case.distinct):
        row = np.concatenate([np.array(sp, np.int64), rng.permutation(other)[: case.fetch_k - len(sp)]])
        out[i] = rng.permutation(row)
    return out


def _list_mid_absent(case, rng, d):
    r = _perm(case, rng, d)
    for i in range(r.shape[0]):
        r[i, rng.choice(np.arange(1, case.fetch_k - 1), size=max(1, case.fetch_k // 4), replace=False)] = -1
    return r


def _list_head_absent(case, rng, d):
    r = _perm(case, rng, d)
    r[:, 0] = -1
    r[1:, 1] = -1                                  # (and a run of two at the head)
    return r


def _list_all_absent(case, rng, d):
    assert case.distinct >= 3
    r = _perm(case, rng, d)
    r[1] = -1                                      # the whole list of query 1; queries 0 and 2 must not notice
    return r


def _list_tail_absent(case, rng, d):
    r = _perm(case, rng, d)
    r[:, case.fetch_k - case.fetch_k // 3:] = -1
    return r


def _list_stale(case, rng, d):
    r = _perm(case, rng, d)
    for i in range(r.shape[0]):
        p = rng.choice(case.fetch_k, size=3, replace=False)
        r[i, p] = [case.n_rows, case.n_rows + 7, 2 ** 40 + i]      # ids past the last row: absent
    return r


def _list_repeat(case, rng, d):
    r = _perm(case, rng, d)
    for i in range(r.shape[0]):
        a, b = rng.choice(case.fetch_k, size=2, replace=False)
        r[i, b] = r[i, a]
    return r


def _list_two_live(case, rng, d):
    r = np.full((case.distinct, case.fetch_k), -1, np.int64)
    for i in range(case.distinct):
        p = rng.choice(case.fetch_k, size=2, replace=False)
        r[i, p] = rng.choice(case.n_rows, size=2, replace=False)
    return r


LIST_BUILDERS = {"perm": _perm, "mid_absent": _list_mid_absent, "head_absent": _list_head_absent, "all_absent": _list_all_absent,
                 "tail_absent": _list_tail_absent, "stale": _list_stale, "repeat": _list_repeat, "two_live": _list_two_live}


def _table():
    c = []

    def add(id, dim, nq, fetch_k, k, lam=0.5, lists="perm", data="random", metric="ip", n_rows=100, tile=0):
        c.append(Case(id, metric, dim, n_rows, nq, fetch_k, k, lam, lists, data, tile))

    # route thresholds: the same call on both sides of dim 384 | 385 and of nq 65535 | 65536
    add("thr-dim384", 384, 5, 20, 10)
    add("thr-dim385", 385, 5, 20, 10)
    add("thr-nq65535", 4, 65535, 4, 2, n_rows=40, tile=16)
    add("thr-nq65536", 4, 65536, 4, 2, n_rows=40, tile=16)
    # k_mmr_lds: every remainder of the 4-way unrolled chain, the empty main loop (dim < 4), the widest rows
    for dim in (1, 2, 3, 4, 5, 7, 383, 384):
        add(f"lds-dim{dim}", dim, 3, 20, 10, data="dim1" if dim == 1 else "random")
    for fk in (1, 2, 20, 63, 64):
        add(f"lds-fk{fk}", 100, 3, fk, 12)
    add("lds-fk64-dim384", 384, 2, 64, 64)                   # the whole LDS area
    # k_mmr: widths, the last workgroup partly empty, list lengths
    for dim in (385, 768, 1024, 3072):
        add(f"wave-dim{dim}", dim, 3, 20, 10)
    for nq in (1, 2, 3, 4, 5):
        add(f"wave-nq{nq}", 400, nq, 20, 10)
    for fk in (1, 20, 64):
        add(f"wave-fk{fk}", 400, 3, fk, 64 if fk == 64 else 12)
    # k against the number of candidates: two live candidates in a list of 20; k = 130 makes the -1 fill loop more than once
    for name, dim in (("lds", 100), ("wave", 400)):
        for k in (1, 20, 70, 130):
            add(f"{name}-k{k}-two-live", dim, 3, 20, k, lists="two_live")
    for name, dim in (("lds", 96), ("wave", 416)):
        for lam in (0.0, 0.35, 0.5, 1.0):
            add(f"{name}-lam{lam:g}", dim, 3, 20, 10, lam=lam)
        for lists in ("mid_absent", "head_absent", "all_absent", "tail_absent", "stale", "repeat"):
            add(f"{name}-list-{lists}", dim, 3, 20, 20 if lists == "repeat" else 10, lists=lists)     # repeat: every candidate is picked, both copies
        for data in ("identical", "zero_row", "zero_query", "near_dup", "pow2"):
            add(f"{name}-data-{data}", dim, 3, 20, 10, lam=0.35 if data == "near_dup" else 0.5, data=data)
    add("lds-data-dim1-lam0.35", 1, 5, 64, 64, lam=0.35, data="dim1")
    # metrics: the kernel reads the STORED rows -- fp32-normalised on a cosine index, 385..768 floats apart on an L2 index
    for name, dim in (("lds", 384), ("wave", 400)):
        for metric in ("ip", "cosine", "l2"):
            add(f"{name}-metric-{metric}", dim, 3, 20, 10, lam=0.35, metric=metric)
        add(f"{name}-metric-cosine-zero-row", dim, 3, 20, 10, metric="cosine", data="zero_row")
    # a removed row that a stale list still names: absent
    for name, dim in (("lds", 128), ("wave", 448)):
        for metric in ("ip", "cosine", "l2"):
            add(f"{name}-removed-{metric}", dim, 4, 20, 10, metric=metric, data="removed")
    assert len({x.id for x in c}) == len(c)
    return c


CASES = _table()
CASE_BY_ID = {c.id: c for c in CASES}


@dataclass
class Built:
    data: Data
    rows: np.ndarray          # [distinct, fetch_k] int64
    q: np.ndarray             # [nq, dim] fp32 (tiled)
    lists: np.ndarray         # [nq, fetch_k] int64 (tiled)


@functools.lru_cache(maxsize=None)
def _build(case_id: str) -> Built:
    case = CASE_BY_ID[case_id]
    assert case.n_rows <= 300 and 1 <= case.fetch_k <= MAX_FETCH_K
    rng = np.random.default_rng(zlib.crc32(case.id.encode()))
    d = DATA_BUILDERS[case.data](case, rng)
    rows = LIST_BUILDERS[case.lists](case, rng, d)
    reps = -(-case.nq // case.distinct)
    q = np.ascontiguousarray(np.tile(d.q, (reps, 1))[: case.nq])
    lists = np.ascontiguousarray(np.tile(rows, (reps, 1))[: case.nq])
    for a in (d.x, d.q, rows, q, lists):
        a.setflags(write=False)
    return Built(d, rows, q, lists)


def build(case: Case) -> Built:
    return _build(case.id)


def normalised(x: np.ndarray) -> np.ndarray:
    """What a cosine index stores, to within an ulp of fp32 (the device sums the squares in another order): x / max(|x|, 1e-12).  The
    CPU test proves its margins on these; the GPU test reads the stored rows back and proves them again on what the kernel really reads."""
    n = np.sqrt((x.astype(np.float32) ** 2).sum(axis=1, dtype=np.float32))
    return (x / np.maximum(n, np.float32(1e-12))[:, None]).astype(np.float32)


def valid_mask(case: Case, ids: np.ndarray, removed=()) -> np.ndarray:
    return (ids >= 0) & (ids < case.n_rows) & ~np.isin(ids, np.asarray(list(removed), np.int64))


@dataclass
class Expect:
    picks: np.ndarray         # [nq, k] int32 (tiled)
    margins: list             # per distinct query: the margins of its picks
    n_decisions: int
    n_ties: int
    unsettled: list           # (query, pick, margin, gap, tied positions) of every decision that is not settled
    min_margin: float         # the smallest margin among the decisions without a tie


def expect(case: Case, stored: np.ndarray | None = None, removed_as_zero_row: bool = False) -> Expect:
    """The reference's answer for a case.  stored: the rows the kernel reads ([n_rows, dim], what rmu_index_get_rows returns; the rows of
    removed ids are never used); default: the rows given (fp32-normalised for a cosine index).  removed_as_zero_row: what a kernel does that
    takes a removed (NaN) row for a candidate whose every cosine is 0 -- the behaviour the removed-row cases must tell from the contract."""
    if stored is None and not removed_as_zero_row:
        return _expect_default(case.id)
    return _expect(case, stored, removed_as_zero_row)


@functools.lru_cache(maxsize=None)
def _expect_default(case_id: str) -> Expect:
    return _expect(CASE_BY_ID[case_id], None, False)


def _expect(case: Case, stored, removed_as_zero_row: bool) -> Expect:
    b = build(case)
    d = b.data
    if stored is None:
        stored = normalised(d.x) if case.metric == "cosine" else d.x
    stored = np.array(stored, dtype=np.float32)
    removed = list(d.removed)
    if removed:
        stored[removed] = 0.0
    picks = np.empty((case.distinct, case.k), np.int32)
    margins, unsettled, n_dec, n_ties, min_margin = [], [], 0, 0, math.inf
    for qi in range(case.distinct):
        ids = b.rows[qi]
        valid = valid_mask(case, ids, () if removed_as_zero_row else removed)
        cand = stored[np.where(valid, ids, 0)]
        p, m, tied, gaps = _greedy(d.q[qi], cand, valid, case.k, case.lam)
        picks[qi] = p
        margins.append(m)

        def label(pos, ids=ids):                          # identical rows, power-of-two copies and a repeated id share a label
            return d.canon.get(int(ids[pos]), int(ids[pos]))

        for t, (mt, tt, gt) in enumerate(zip(m, tied, gaps)):
            n_dec += 1
            n_ties += bool(tt)
            if not tt:
                min_margin = min(min_margin, mt)
            if case.dim == 1 or (qi in d.zero_q and t == 0):
                ok = settled(mt, gt, tt, lambda pos: 0)         # one class for every candidate
            else:
                ok = settled(mt, gt, tt, label)
            if not ok:
                unsettled.append((qi, t, mt, gt, tt))
    reps = -(-case.nq // case.distinct)
    return Expect(np.ascontiguousarray(np.tile(picks, (reps, 1))[: case.nq]), margins, n_dec, n_ties, unsettled, min_margin)


# ---- running a case on the device ----------------------------------------------------------------------------------------------------
def _metric(name: str) -> int:
    from ragmeup_amd import _native as N
    return {"ip": N.METRIC_IP, "cosine": N.METRIC_COSINE, "l2": N.METRIC_L2SQ}[name]


def make_index(rmu, case: Case):
    """The index of a case and the rows it stores: bit for bit the rows given on an ip / l2 index, the fp32-normalised rows on a cosine
    index (a zero row stays zero); the rows of removed ids are left out (zero here, never used)."""
    b = build(case)
    idx = rmu.FlatIndex(case.dim, metric=_metric(case.metric), capacity_hint=case.n_rows)
    idx.add(b.data.x)
    live = np.array([r for r in range(case.n_rows) if r not in set(b.data.removed)], np.int64)
    if b.data.removed:
        assert idx.remove_rows(np.array(b.data.removed, np.int64)) == len(b.data.removed)
    stored = np.zeros((case.n_rows, case.dim), np.float32)
    stored[live] = idx.get_rows(live)
    return idx, stored


def stored_diff(case: Case, stored: np.ndarray) -> list:
    x = build(case).data.x
    live = np.array([r for r in range(case.n_rows) if r not in set(build(case).data.removed)], np.int64)
    if case.metric != "cosine":
        return [] if np.array_equal(stored[live].view(np.uint32), x[live].view(np.uint32)) else ["the stored rows are not the rows given"]
    n = np.linalg.norm(stored[live].astype(np.float64), axis=1)
    zero = ~x[live].any(axis=1)
    ok = (np.abs(n[~zero] - 1.0) < 1e-6).all() and not stored[live][zero].any() and np.allclose(stored[live], normalised(x[live]), rtol=0, atol=1e-6)
    return [] if ok else ["the stored rows of the cosine index are not the normalised rows"]


def call_mmr(lib, idx, case: Case, device: bool = False) -> tuple:
    """rmu_index_mmr on a case's queries and lists -> (out_pos [nq, k] int32, guard [k] int32): the output starts filled with FILL_POS and has
    one guard row behind it.  device: q, the lists and out_pos are torch tensors on the device (RMU_F_Q_DEVICE | RMU_F_OUT_DEVICE)."""
    b = build(case)
    out = np.full((case.nq + 1, case.k), FILL_POS, np.int32)
    if device:
        import torch
        dev = torch.device("cuda", 0)
        q_d, r_d, o_d = torch.tensor(b.q, device=dev), torch.tensor(b.lists, device=dev), torch.tensor(out, device=dev)
        torch.cuda.synchronize()
        rc = lib.rmu_index_mmr(idx._h, q_d.data_ptr(), case.nq, r_d.data_ptr(), case.fetch_k, case.k, float(case.lam),
                               F_Q_DEVICE | F_OUT_DEVICE, o_d.data_ptr())
        torch.cuda.synchronize()
        out = o_d.cpu().numpy()
    else:
        rc = lib.rmu_index_mmr(idx._h, b.q.ctypes.data, case.nq, b.lists.ctypes.data, case.fetch_k, case.k, float(case.lam), 0, out.ctypes.data)
    assert rc == 0, (case.id, rc, lib.rmu_last_error())
    return out[: case.nq], out[case.nq]


def run_case(rmu, case: Case, device: bool = False):
    """-> (diff, out_pos): diff is empty when the device's picks equal the reference's on the rows the index stores, every slot was written,
    the guard row was not, and every decision of the reference on those rows is settled."""
    from ragmeup_amd import _native
    idx, stored = make_index(rmu, case)
    try:
        got, guard = call_mmr(_native.lib(), idx, case, device)
    finally:
        idx.close()
    diff = stored_diff(case, stored)
    want = expect(case, None if case.metric != "cosine" else stored)
    if want.unsettled:
        diff.append(f"unsettled decisions on the stored rows: {want.unsettled[:3]}")
    if (guard != FILL_POS).any():
        diff.append(f"the guard row behind the output was written: {guard.tolist()[:8]}")
    if (got == FILL_POS).any():
        diff.append(f"{int((got == FILL_POS).sum())} slots were not written, first at {np.argwhere(got == FILL_POS)[0].tolist()}")
    bad = np.flatnonzero((got != want.picks).any(axis=1))
    for qi in bad[:3]:
        diff.append(f"query {int(qi)}: got {got[qi].tolist()[:24]} want {want.picks[qi].tolist()[:24]}")
    if bad.size > 3:
        diff.append(f"... and {bad.size - 3} more queries")
    return diff, got


def run_all(rmu) -> dict:
    """Every case and one search + selection in one call at dim 384 (launch_mmr behind rmu_index_search_mmr): the cases that differ from
    the reference, the routes taken, and a digest of every answer.  tests/mmr_variant_driver.py prints this for the process it runs in."""
    lds_on = lds_on_in_this_process()
    failed, routes, sha = {}, set(), hashlib.sha1()
    for case in CASES:
        r = route(case.dim, case.nq, lds_on)
        routes.add(r)
        diff, got = run_case(rmu, case)
        sha.update(np.ascontiguousarray(got).tobytes())
        if diff:
            failed[case.id] = [r] + diff
    rng = np.random.default_rng(384)
    x = rng.standard_normal((300, 384)).astype(np.float32)
    q = (x[:7] + 0.6 * rng.standard_normal((7, 384))).astype(np.float32)
    idx = rmu.FlatIndex(384, capacity_hint=300)
    try:
        idx.add(x)
        rows, sc = idx.search_mmr(q, 20, 10, 0.35, row_base=1000)
        s2, r2 = idx.search(q, 20)
        pos = idx.mmr(q, r2, 10, 0.35)
    finally:
        idx.close()
    routes.add(route(384, 7, lds_on))
    search_ok = bool((rows == np.take_along_axis(r2, pos.astype(np.int64), axis=1) + 1000).all()
                     and (sc == np.take_along_axis(s2, pos.astype(np.int64), axis=1)).all())
    sha.update(rows.tobytes() + sc.tobytes())
    return {"lds_on": lds_on, "cases": len(CASES), "failed": failed, "routes": sorted(routes), "search_ok": search_ok, "digest": sha.hexdigest()}

