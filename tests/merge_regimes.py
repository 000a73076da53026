"""The top-k merge (ragmeup_amd/csrc/topk_merge.hip) restated in numpy: the key codec of rmu_common.h, exact references for the key
merges and for the generic list merge, the launcher's dispatch (`route`), the three launchers as ctypes functions, builders of part
lists, and the table of cases that holds every kernel, instantiation and guard from both sides of its threshold.

A plain helper module, not a fixture: tests/test_merge_regimes_cpu.py reads every constant below back out of the source and checks that
CASES reaches every route and threshold; tests/test_merge_regimes_gpu.py runs CASES and LIST_CASES on the device, and
tests/merge_variant_driver.py runs the key-merge cases once more in a process whose merges all go through merge_wg_kernel
(RMU_TUNING=1 RMU_MERGE_SELECT=0).  The merge is integer code over u64 keys: every reference here is exact and every comparison is
equality.

A key is (rmu_f2ord(score) << 32) | ~row: descending key order is (score descending, row ascending), 0 is the empty slot.  The scans
emit distinct keys (a row appears once per query); the selection kernel's tau step relies on it and so do the builders.
"""
from __future__ import annotations

import ctypes
import zlib
from dataclasses import dataclass

import numpy as np

# ---- constants of topk_merge.hip (tests/test_merge_regimes_cpu.py reads them back) ----------------------------------------------------
MAX_K = 128                   # k > 128 is refused
SELECT_SMALL_K = 32           # k <= 32: merge_select_kernel<*, 1024>; above: <*, 3072>
SELECT_MAX_PARTS = 1024       # parts <= 1024 (= MAXP, the heads array): selection; above: merge_wg_kernel
SELECT_WIDE_NQ = 512          # nq <= 512: 1024 threads per query; above: 256
BLOCK_WIDE, BLOCK_NARROW = 1024, 256
CAPM_SMALL, CAPM_DEEP = 1024, 3072
MAXP = 1024
WG_WAVES = 16                 # waves of a merge_wg_kernel workgroup = the largest wpq
WG_PARTS_PER_WAVE = 16        # first loop: wpq doubles while parts > 16 * wpq
WG_MIN_WAVES = 2048           # second loop: ... while nq * wpq < 2048 and wpq < parts
NPL1_MAX_K = 64               # k <= 64: one key per lane (NPL = 1); above: two
BATCH = 64                    # keys per sort batch (one per lane)
SLAB = 4                      # ranks per slab
E_INVALID, E_HIP = -1, -2

FILL_BITS = np.uint32(0x7FC0BEEF)      # a NaN pattern no kernel writes: "this score was not written"
FILL_ROW = np.int64(-7)
FILL_KEY = np.uint64(0xDEADBEEFDEADBEEF)
U32, U64 = np.uint32, np.uint64


# ---- key codec (rmu_common.h) -----------------------------------------------------------------------------------------------------
def f2ord(f):
    u = np.ascontiguousarray(f, dtype=np.float32).view(U32)
    return u ^ np.where(u >> U32(31), U32(0xFFFFFFFF), U32(0x80000000))


def ord2f(o):
    o = np.ascontiguousarray(o, dtype=U32)
    return (o ^ np.where(o >> U32(31), U32(0x80000000), U32(0xFFFFFFFF))).view(np.float32)


def make_key(score, row):
    return (f2ord(score).astype(U64) << U64(32)) | (~np.asarray(row).astype(U32)).astype(U64)


def key_score(key):
    return ord2f((np.asarray(key, dtype=U64) >> U64(32)).astype(U32))


def key_row(key):
    return ~(np.asarray(key, dtype=U64) & U64(0xFFFFFFFF)).astype(U32)


# ---- references --------------------------------------------------------------------------------------------------------------------
def ref_keys(lists, k: int):
    """[parts, nq, k] u64 part lists -> [nq, k] merged keys: the k largest non-zero keys of each query, descending, 0-padded."""
    parts, nq, kk = lists.shape
    assert kk == k and lists.dtype == U64
    flat = np.transpose(lists, (1, 0, 2)).reshape(nq, parts * k)
    return np.ascontiguousarray(np.sort(flat, axis=1)[:, ::-1][:, :k])           # (zeros are the smallest u64: they sort last)


def ref_final(lists, k: int, row_base: int = 0, l2_out: bool = False, qn=None, scatter=None, n_out: int | None = None, cond=None):
    """rmu_merge_final_launch: (score bit patterns [n_out, k] u32, rows [n_out, k] i64), starting from the fills.  `scatter`: query i
    writes output row scatter[i]; `qn` (l2_out) is indexed by the OUTPUT row.  `cond` = (c, lo, hi, clamp): c outside [lo, hi] ->
    nothing is written; clamp -> only the first min(c, nq) queries are merged."""
    parts, nq, _ = lists.shape
    n_out = nq if n_out is None else n_out
    bits = np.full((n_out, k), FILL_BITS, U32)
    rows = np.full((n_out, k), FILL_ROW, np.int64)
    nq_eff = nq
    if cond is not None:
        c, lo, hi, clamp = cond
        if c < lo or c > hi:
            return bits, rows
        if clamp and c < nq:
            nq_eff = max(c, 0)
    if nq_eff == 0:
        return bits, rows
    keys = ref_keys(lists, k)[:nq_eff]
    qo = np.arange(nq_eff) if scatter is None else np.asarray(scatter, np.int64)[:nq_eff]
    s = key_score(keys)
    if l2_out:
        s = np.maximum(np.asarray(qn, np.float32)[qo][:, None] - s, np.float32(0))     # one fp32 subtraction: bit-exact
    empty = keys == 0
    s = np.where(empty, np.float32(np.inf if l2_out else -np.inf), s).astype(np.float32)
    r = np.where(empty, np.int64(-1), key_row(keys).astype(np.int64) + np.int64(row_base))
    bits[qo] = s.view(U32)
    rows[qo] = r
    return bits, rows


def ref_to_keys(lists, k: int, seed_init=None):
    """rmu_merge_to_keys_launch: (keys [nq, k], seed_thr [nq] or None).  seed_thr[q] = max(seed_thr[q], image of the merged k-th best),
    left alone when the k-th slot is empty."""
    keys = ref_keys(lists, k)
    if seed_init is None:
        return keys, None
    kth = keys[:, k - 1]
    img = (kth >> U64(32)).astype(U32)
    return keys, np.where(kth != 0, np.maximum(np.asarray(seed_init, U32), img), np.asarray(seed_init, U32)).astype(U32)


def ref_lists(scores, rows, k: int, smaller_better: bool):
    """merge_lists_kernel over [parts, nq, k] (scores fp32, rows i64): candidates with row < 0 or a NaN score are dropped; the rest is
    ordered by score (direction by `smaller_better`), equal scores -- +0 and -0 are equal -- by candidate index, i.e. lower part, then
    earlier position; padding is (-inf, -1), or (+inf, -1) for distances.  Returns (scores [nq, k] fp32, rows [nq, k] i64, candidate
    index [nq, k], -1 in the padding)."""
    parts, nq, kk = scores.shape
    assert kk == k
    out_s = np.full((nq, k), np.inf if smaller_better else -np.inf, np.float32)
    out_r = np.full((nq, k), -1, np.int64)
    out_i = np.full((nq, k), -1, np.int64)
    for q in range(nq):
        s = scores[:, q, :].reshape(-1)
        r = rows[:, q, :].reshape(-1)
        cand = np.nonzero((r >= 0) & ~np.isnan(s))[0]
        sc = s[cand].astype(np.float64)
        order = cand[np.argsort(sc if smaller_better else -sc, kind="stable")][:k]
        out_s[q, :order.size], out_r[q, :order.size], out_i[q, :order.size] = s[order], r[order], order
    return out_s, out_r, out_i


# ---- the dispatch of merge_wg_launch ---------------------------------------------------------------------------------------------
def wpq_of(parts: int, nq: int) -> int:
    wpq = 1
    while wpq < WG_WAVES and parts > WG_PARTS_PER_WAVE * wpq:
        wpq <<= 1
    while wpq < WG_WAVES and nq * wpq < WG_MIN_WAVES and wpq < parts:
        wpq <<= 1
    return wpq


def route(parts: int, nq: int, k: int, select: bool = True) -> tuple:
    """Which kernel serves a key merge: ("invalid",), ("select", BLOCK, CAPM) or ("wg", NPL, wpq).  `select` False: the process runs
    with RMU_TUNING=1 RMU_MERGE_SELECT=0."""
    if k < 1 or k > MAX_K or parts < 1 or nq < 1:
        return ("invalid",)
    if select and parts <= SELECT_MAX_PARTS:
        return ("select", BLOCK_WIDE if nq <= SELECT_WIDE_NQ else BLOCK_NARROW, CAPM_SMALL if k <= SELECT_SMALL_K else CAPM_DEEP)
    return ("wg", 1 if k <= NPL1_MAX_K else 2, wpq_of(parts, nq))


def count_ge_tau(lists, k: int):
    """Per query, the number of keys merge_select_kernel appends to its candidate array: tau = the k-th largest list head (0 when
    parts < k or fewer than k lists hold a key), count = the non-zero keys >= tau.  count > CAPM sends the query to the fallback."""
    parts, nq, _ = lists.shape
    heads = lists.max(axis=2)                                        # [parts, nq]
    tau = np.sort(heads, axis=0)[::-1][k - 1] if parts >= k else np.zeros(nq, U64)
    return ((lists != 0) & (lists >= tau[None, :, None])).sum(axis=(0, 2))


# ---- the launchers -------------------------------------------------------------------------------------------------------------------
class RmuCond(ctypes.Structure):
    _fields_ = [("p", ctypes.c_void_p), ("lo", ctypes.c_int), ("hi", ctypes.c_int), ("clamp", ctypes.c_int)]


_vp, _i32, _i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
# C++ names: librmu.so is built without -fvisibility=hidden, the launchers of rmu_common.h are exported as they are mangled
SYMBOLS = {
    # (partial, parts, nq, k, row_base, l2_out, qnorm2, out_scores, out_rows, scatter, cond, stream)
    "final": ("_Z22rmu_merge_final_launchPKyililiPKfPfPlPKlPK7RmuCondP12ihipStream_t",
              [_vp, _i32, _i64, _i32, _i64, _i32, _vp, _vp, _vp, _vp, ctypes.POINTER(RmuCond), _vp]),
    # (partial, parts, nq, k, out_keys, seed_thr, stream, unsorted)
    "to_keys": ("_Z24rmu_merge_to_keys_launchPKyiliPyPjP12ihipStream_ti", [_vp, _i32, _i64, _i32, _vp, _vp, _vp, _i32]),
    # (scores, rows, parts, stride_s, stride_r, nq, k, smaller_better, out_scores, out_rows, stream)
    "lists": ("_Z22rmu_merge_lists_launchPKfPKlillliiPfPlP12ihipStream_t", [_vp, _vp, _i32, _i64, _i64, _i64, _i32, _i32, _vp, _vp, _vp]),
}


def launchers(lib) -> dict:
    """{"final", "to_keys", "lists"} -> the ctypes function of a loaded librmu.so."""
    out = {}
    for name, (sym, argtypes) in SYMBOLS.items():
        try:
            fn = getattr(lib, sym)
        except AttributeError:
            raise RuntimeError(f"librmu.so does not export {sym}: the signature of the {name} launcher in topk_merge.hip changed, or the "
                               f"library is built with hidden visibility -- update SYMBOLS in tests/merge_regimes.py") from None
        fn.argtypes, fn.restype = argtypes, ctypes.c_int
        out[name] = fn
    return out


# ---- part lists --------------------------------------------------------------------------------------------------------------------
def _fill_full(rng, parts, nq, k):
    return np.full((parts, nq), k, np.int64)


def _fill_mixed(rng, parts, nq, k):
    """any number of keys per list; list 0 of query 0 full"""
    c = rng.integers(0, k + 1, (parts, nq))
    c[0, 0] = k
    return c


def _fill_sparse(rng, parts, nq, k):
    """What a seeded ladder launch leaves: 1..3 keys in most lists, none in a fifth of them.  Query 1 (if there is one): every list empty.
    Query 2: fewer than k lists hold a key, so that tau = 0 although parts >= k."""
    c = np.minimum(rng.integers(1, 4, (parts, nq)), k) * (rng.random((parts, nq)) > 0.2)
    if nq >= 2:
        c[:, 1] = 0
    if nq >= 3 and k >= 2:
        keep = rng.permutation(parts)[:k - 1]
        only = np.zeros(parts, bool)
        only[keep] = True
        c[:, 2] = np.where(only, np.maximum(c[:, 2], 1), 0)
    return c


def _fill_lens(rng, parts, nq, k):
    """lists of 1, 4, 5, k, 0 and k - 1 keys, in turn"""
    lens = np.array([1, min(4, k), min(5, k), k, 0, k - 1])
    return lens[(np.arange(parts)[:, None] + np.arange(nq)[None, :]) % 6]


def _fill_wg(rng, parts, nq, k):
    """Query 0: every key in the parts of ONE `sub` wave at wpq = 16 (parts = 5 mod 16).  Query 1: fewer than k keys in total, one per
    list.  The others: any number per list."""
    c = rng.integers(0, k + 1, (parts, nq))
    c[:, 0] = np.where(np.arange(parts) % 16 == 5, k, 0)
    if nq >= 2:
        c[:, 1] = 0
        c[rng.permutation(parts)[:max(k - 2, 1)], 1] = 1
    return c


def _fill_cap_at(rng, parts, nq, k):
    assert parts * k == CAPM_DEEP
    return np.full((parts, nq), k, np.int64)


def _fill_cap_over(rng, parts, nq, k):
    """(parts - 1) * k = CAPM full lists; the last list holds ONE key for query 0 (CAPM + 1 keys: fallback) and none for the others"""
    assert (parts - 1) * k == CAPM_DEEP
    c = np.full((parts, nq), k, np.int64)
    c[-1, :] = 0
    c[-1, 0] = 1
    return c


def _fill_tau_low(rng, parts, nq, k):
    """parts == k full lists except the last, which holds one key -- the lowest of the query (`low_last`): tau is that key"""
    assert parts == k
    c = np.full((parts, nq), k, np.int64)
    c[-1, :] = 1
    return c


FILLS = {"full": _fill_full, "mixed": _fill_mixed, "sparse": _fill_sparse, "lens": _fill_lens, "wg": _fill_wg, "cap_at": _fill_cap_at,
         "cap_over": _fill_cap_over, "tau_low": _fill_tau_low}


def build_lists(parts: int, nq: int, k: int, counts, rng, unsorted: bool = False, ties: bool = False, low_last: bool = False):
    """[parts, nq, k] u64 part lists with counts[p, q] keys in list (p, q), distinct within a query.
    sorted form: descending, zeros last.  unsorted: compact (zeros last), the occupied slots in random order with the list's BEST key in
    its LAST occupied slot.  ties: scores on a grid of 1/4 (many equal scores, +0 and -0 among them; rows break the ties).
    low_last: the keys of the last part are the lowest of their query.  Rows: 0 .. parts * k - 1 per query, the largest replaced by
    2^32 - 2 (the largest row a key can carry next to the empty slot's image)."""
    m = parts * k
    s = rng.standard_normal((nq, m), dtype=np.float32)
    if ties:
        s = (np.round(s * 4) / 4).astype(np.float32)
    rows = rng.permuted(np.tile(np.arange(m, dtype=np.int64), (nq, 1)), axis=1)
    rows[rows == m - 1] = 2 ** 32 - 2
    s = np.transpose(s.reshape(nq, parts, k), (1, 0, 2))
    rows = np.transpose(rows.reshape(nq, parts, k), (1, 0, 2))
    if low_last:
        s = s.copy()
        s[-1] -= np.float32(100.0)
    keys = np.sort(make_key(s, rows), axis=2)[:, :, ::-1].copy()
    pos = np.arange(k)[None, None, :]
    cnt = np.asarray(counts, np.int64)[:, :, None]
    keys[pos >= cnt] = 0
    if unsorted:
        r = rng.random((parts, nq, k))
        r = np.where(pos >= cnt, 2.0, np.where(pos == 0, 1.5, r))            # the others (any order), then the best, then the zeros
        keys = np.take_along_axis(keys, np.argsort(r, axis=2, kind="stable"), axis=2)
    return np.ascontiguousarray(keys)


# ---- the cases ------------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    id: str
    parts: int
    nq: int
    k: int
    fill: str = "full"
    unsorted: bool = False        # compact shuffled lists, merged with unsorted = 1 (rmu_merge_to_keys_launch only)
    ties: bool = False
    low_last: bool = False
    # MergeOut of the final launch
    row_base: int = 0
    scatter: bool = False         # a permutation into an output of nq + 3 rows
    l2: bool = False
    cond: tuple = ()              # (c, lo, hi, clamp)
    cap: str = ""                 # where a query of the case takes count_ge_tau: "" every query below CAPM, "at" (== CAPM, none above), "over"

    @property
    def route(self):
        return route(self.parts, self.nq, self.k)

    @property
    def route_wg(self):
        return route(self.parts, self.nq, self.k, select=False)


@dataclass
class Built:
    lists: np.ndarray             # [parts, nq, k] u64
    n_out: int                    # rows of the final launch's output
    scatter: np.ndarray | None    # [nq] i64
    qn: np.ndarray | None         # [n_out] fp32
    seed_init: np.ndarray         # [nq] u32: per query above / below / equal to the merged k-th image, or 0
    cond: tuple | None


def build(case: Case) -> Built:
    rng = np.random.default_rng(zlib.crc32(case.id.encode()))
    counts = FILLS[case.fill](rng, case.parts, case.nq, case.k)
    lists = build_lists(case.parts, case.nq, case.k, counts, rng, unsorted=case.unsorted, ties=case.ties, low_last=case.low_last)
    n_out = case.nq + 3 if case.scatter else case.nq
    scatter = rng.permutation(n_out)[:case.nq].astype(np.int64) if case.scatter else None
    merged = ref_keys(lists, case.k)
    qn = None
    if case.l2:
        # |q|^2 of an output row = the score in the MIDDLE of the list merged into it: qn - s is negative above it (the clamp acts), zero at
        # it and positive below.  (No grid scores here: fmaxf(-0, +0) may return either zero.)
        assert not case.ties
        qn = np.float32(0.25) + rng.random(n_out, dtype=np.float32)
        mid = merged[:, case.k // 2]
        qo = np.arange(case.nq) if scatter is None else scatter
        qn[qo[mid != 0]] = key_score(mid[mid != 0])
    kth = (merged[:, case.k - 1] >> U64(32)).astype(np.int64)
    delta = np.array([1, -1, 0, 0])[np.arange(case.nq) % 4]
    seed = np.where(np.arange(case.nq) % 4 == 3, 0, np.clip(kth + delta, 0, 2 ** 32 - 1)).astype(U32)
    return Built(lists=lists, n_out=n_out, scatter=scatter, qn=qn, seed_init=seed, cond=case.cond or None)


def _c(id_, parts, nq, k, fill="full", **kw):
    return Case(id_, parts, nq, k, fill, **kw)


CASES = (
    # 1. selection, k <= 32 (<1024, 1024> and <256, 1024>): parts around k, parts not a multiple of 16, k not a multiple of 4
    [_c(f"sel-k{k}-p{p}-nq{nq}-{fill}", p, nq, k, fill, ties=(k % 2 == 1))
     for k, p, nq, fill in (
         (1, 1, 1, "full"), (1, 2, 5, "mixed"), (1, 17, 5, "sparse"),
         (3, 2, 5, "full"), (3, 3, 1, "full"), (3, 4, 5, "mixed"), (3, 250, 5, "sparse"),
         (10, 1, 5, "mixed"), (10, 9, 5, "full"), (10, 10, 5, "full"), (10, 11, 5, "full"), (10, 17, 512, "mixed"), (10, 17, 513, "mixed"),
         (10, 250, 5, "sparse"), (10, 1024, 1, "mixed"), (10, 1024, 5, "sparse"),
         (31, 30, 5, "full"), (31, 31, 5, "mixed"), (31, 32, 1, "full"), (31, 250, 5, "sparse"),
         (32, 31, 5, "full"), (32, 32, 5, "full"), (32, 33, 5, "mixed"), (32, 17, 513, "sparse"), (32, 1024, 1, "sparse"))]
    # 2. selection, 33 <= k <= 128 (<*, 3072>), the candidate count on both sides of CAPM
    + [_c(f"deep-k{k}-p{p}-nq{nq}-{fill}", p, nq, k, fill, ties=(k % 2 == 1))
       for k, p, nq, fill in ((33, 5, 513, "mixed"), (33, 34, 5, "full"), (64, 17, 5, "mixed"), (65, 66, 1, "full"), (65, 250, 5, "sparse"),
                              (100, 13, 5, "lens"), (127, 126, 1, "sparse"), (127, 128, 5, "sparse"), (128, 130, 2, "full"), (128, 1024, 1, "sparse"))]
    + [_c("deep-k128-p24-count3072", 24, 2, 128, "cap_at", cap="at"),
       _c("deep-k127-p126-mixed-fallback", 126, 1, 127, "mixed", ties=True, cap="over"),
       _c("deep-k128-p25-count3073", 25, 2, 128, "cap_over", cap="over"),
       _c("deep-k128-p128-tau-low", 128, 2, 128, "tau_low", low_last=True, cap="over"),
       _c("deep-k100-p40-full-fallback", 40, 3, 100, "full", cap="over")]
    # 3. unsorted = 1: compact shuffled lists, the best key of a list in its last occupied slot
    + [_c(f"unsorted-k{k}-p{p}-nq{nq}-{fill}", p, nq, k, fill, unsorted=True, ties=(k == 10))
       for k, p, nq, fill in ((10, 17, 5, "lens"), (10, 33, 513, "sparse"), (32, 33, 5, "lens"), (32, 16, 3, "full"), (40, 41, 5, "lens"),
                              (40, 7, 3, "mixed"), (128, 13, 3, "lens"), (128, 130, 2, "full"))]
    + [_c("unsorted-k128-p24-count3072", 24, 2, 128, "cap_at", unsorted=True, cap="at"),
       _c("unsorted-k128-p25-count3073", 25, 2, 128, "cap_over", unsorted=True, cap="over"),
       _c("unsorted-k10-p1025-lens", 1025, 2, 10, "lens", unsorted=True),
       _c("unsorted-k128-p1025-lens", 1025, 1, 128, "lens", unsorted=True)]
    # 4. merge_wg_kernel in the default process (parts > 1024: wpq = 16)
    + [_c(f"wg-k{k}-p{p}-nq{nq}-{fill}", p, nq, k, fill, ties=(k % 2 == 1))
       for k, p, nq, fill in ((5, 1025, 3, "wg"), (5, 1040, 1, "sparse"), (64, 1025, 1, "mixed"), (64, 1040, 3, "wg"), (65, 1025, 3, "wg"),
                              (65, 1040, 1, "full"), (128, 1025, 1, "sparse"), (128, 1040, 3, "wg"))]
    # ... and the shapes that give it every wpq when the selection is switched off (they are selection cases in the default process)
    + [_c(f"wpq-k{k}-p{p}-nq{nq}-{fill}", p, nq, k, fill)
       for k, p, nq, fill in ((3, 16, 2048, "mixed"), (3, 16, 2047, "mixed"), (10, 17, 1024, "sparse"), (10, 33, 512, "mixed"), (10, 65, 256, "sparse"),
                              (65, 1, 5, "full"), (65, 2, 5, "full"), (65, 3, 5, "mixed"), (100, 7, 5, "mixed"), (65, 16, 128, "sparse"), (70, 32, 64, "sparse"), (70, 33, 64, "sparse"),
                              (10, 64, 32, "mixed"), (10, 128, 16, "sparse"), (10, 129, 16, "sparse"))]
    # 5. MergeOut, each field on a selection case and on a merge_wg case
    + [_c(f"out-{tag}-{name}", p, nq, k, fill, **kw)
       for tag, (p, nq, k, fill) in (("sel", (17, 6, 10, "mixed")), ("wg", (1025, 6, 10, "wg")))
       for name, kw in (("rowbase", dict(row_base=1_000_000_007)),
                        ("scatter", dict(scatter=True)),
                        ("l2", dict(l2=True)),
                        ("scatter-l2-rowbase", dict(scatter=True, l2=True, row_base=5_000_000_000)),
                        ("cond-below", dict(cond=(2, 3, 6, 1))),
                        ("cond-above", dict(cond=(7, 3, 6, 1))),
                        ("cond-lo-clamp", dict(cond=(3, 3, 6, 1), scatter=True)),
                        ("cond-hi-clamp", dict(cond=(5, 1, 5, 1))),
                        ("cond-inside-noclamp", dict(cond=(2, 1, 0x7FFFFFFF, 0))))]
    + [_c("out-deep-scatter-l2", 25, 2, 128, "cap_over", scatter=True, l2=True, row_base=77, cap="over"),       # the fallback's emit
       _c("out-deep-cond-clamp", 13, 6, 40, "mixed", cond=(4, 1, 6, 1), l2=True)]
)

# (k, parts, nq) the launchers must refuse with RMU_E_INVALID, launching nothing
REFUSED = [(0, 4, 3), (129, 4, 3), (10, 0, 3), (10, 4, 0), (-1, 4, 3), (10, -2, 3)]
REFUSED_LISTS_ONLY = [(128, 1 << 25, 1)]            # parts * k = 2^32: a candidate index no longer fits the key's row field


# ---- merge_lists_kernel ---------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class ListCase:
    id: str
    parts: int
    nq: int
    k: int
    smaller_better: bool
    layout: str                   # "packed": part p at p * nq * k;  "padded": strides larger than nq * k, two buffers;
                                  # "comm": ONE buffer of [scores | rows] blocks per part, as rmu_comm.hip receives them


LIST_CASES = [ListCase(f"lists-k{k}-p{p}-nq{nq}-{'dist' if sb else 'sim'}-{lay}", p, nq, k, sb, lay)
              for k, p, nq, sb, lay in (
                  (1, 1, 1, False, "packed"), (1, 13, 7, True, "comm"), (10, 2, 4, False, "comm"), (10, 8, 7, True, "padded"), (10, 13, 1, False, "padded"),
                  (64, 1, 4, True, "packed"), (64, 2, 7, False, "comm"), (64, 13, 4, True, "packed"), (65, 1, 7, False, "padded"), (65, 8, 1, True, "comm"),
                  (65, 13, 4, False, "packed"), (128, 2, 7, True, "padded"), (128, 8, 4, False, "comm"), (128, 13, 7, True, "comm"), (10, 8, 4, True, "packed"))]


def build_list_case(case: ListCase):
    """(scores [parts, nq, k] fp32, rows [parts, nq, k] i64): scores on a grid of 1/2 (duplicates inside and across parts), with +0, -0,
    +inf, -inf next to valid rows, NaN next to valid rows (dropped) and next to -1, and (-inf | +inf, -1) padding at the end of some
    lists.  The lists are NOT sorted: the kernel sorts every candidate, the order of its input decides ties only."""
    rng = np.random.default_rng(zlib.crc32(case.id.encode()))
    shape = (case.parts, case.nq, case.k)
    s = (np.round(rng.standard_normal(shape) * 2) / 2).astype(np.float32)
    special = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 0.0, -0.0], np.float32)
    pick = rng.random(shape) < 0.25
    s[pick] = special[rng.integers(0, special.size, int(pick.sum()))]
    rows = rng.integers(0, 2 ** 40, shape, dtype=np.int64)
    rows[rng.random(shape) < 0.05] = -1                                   # a hole anywhere in a list (any score beside it)
    pad = rng.integers(0, case.k + 1, shape[:2]) * (rng.random(shape[:2]) < 0.4)      # the last `pad` slots of a list are padding
    is_pad = np.arange(case.k)[None, None, :] >= (case.k - pad)[:, :, None]
    rows[is_pad] = -1
    s[is_pad] = np.inf if case.smaller_better else -np.inf
    if case.nq >= 4:                                                      # one query without any candidate
        rows[:, 3, :] = -1
    return s, rows


def lay_out(case: ListCase, s, rows):
    """-> (buffers, scores offset, rows offset, stride_s, stride_r): `buffers` is a list of one or two numpy arrays to place on the
    device; offsets are in bytes into buffers[0] (scores) and buffers[-1] (rows); strides in elements, as the launcher takes them."""
    n = case.nq * case.k
    if case.layout == "packed":
        return [s.reshape(-1).copy(), rows.reshape(-1).copy()], 0, 0, n, n
    if case.layout == "padded":
        ss, sr = n + 5, n + 3
        bs = np.full(case.parts * ss, np.float32(np.nan), np.float32)
        br = np.full(case.parts * sr, 12345, np.int64)                  # (a valid row beside a NaN score: dropped if it were ever read)
        for p in range(case.parts):
            bs[p * ss:p * ss + n] = s[p].reshape(-1)
            br[p * sr:p * sr + n] = rows[p].reshape(-1)
        return [bs, br], 0, 0, ss, sr
    rows_off = (n * 4 + 7) & ~7                                          # rmu_comm.hip: [scores | rows] per rank, rows 8-byte aligned
    per_rank = rows_off + n * 8
    buf = np.zeros(case.parts * per_rank, np.uint8)
    for p in range(case.parts):
        buf[p * per_rank:p * per_rank + n * 4] = s[p].reshape(-1).view(np.uint8)
        buf[p * per_rank + rows_off:(p + 1) * per_rank] = rows[p].reshape(-1).view(np.uint8)
    assert per_rank % 8 == 0
    return [buf], 0, rows_off, per_rank // 4, per_rank // 8


# ---- running a case on the device (shared by tests/test_merge_regimes_gpu.py and tests/merge_variant_driver.py) ------------------------
def _first_diff(name, got, want, show=lambda v: v):
    if np.array_equal(got, want):
        return []
    at = tuple(int(v) for v in np.argwhere(got != want)[0])
    return [f"{name}: {int((got != want).sum())} entries differ, first at {at}: got {show(got[at])}, expected {show(want[at])}"]


def _show_key(key):
    key = np.uint64(key)
    return f"{int(key):#018x} (score {float(key_score(key)[0])!r}, row {int(key_row(key)[0])})" if key else "0 (empty)"


def run_key_case(fns, case: Case, built: Built | None = None) -> list:
    """Runs the case through rmu_merge_to_keys_launch (keys and seed_thr) and, for sorted lists, through rmu_merge_final_launch (scores
    and rows with the case's MergeOut fields) on cuda:0, and compares WHOLE output arrays -- the regions nobody may write included --
    with the references.  Returns the list of differences, empty when the case passes."""
    import torch
    b = built or build(case)
    parts, nq, k = case.parts, case.nq, case.k
    dev = torch.device("cuda", 0)
    put = lambda a, view: torch.from_numpy(np.ascontiguousarray(a).view(view)).to(dev)
    lists_d = put(b.lists, np.int64)
    out = []
    keys_d = put(np.full((nq, k), FILL_KEY, U64), np.int64)
    seed_d = put(b.seed_init, np.int32)
    torch.cuda.synchronize()
    rc = fns["to_keys"](lists_d.data_ptr(), parts, nq, k, keys_d.data_ptr(), seed_d.data_ptr(), None, int(case.unsorted))
    torch.cuda.synchronize()
    want_keys, want_seed = ref_to_keys(b.lists, k, b.seed_init)
    if rc != 0:
        out.append(f"to_keys: rc = {rc}")
    out += _first_diff("to_keys: keys", keys_d.cpu().numpy().view(U64), want_keys, _show_key)
    out += _first_diff("to_keys: seed_thr", seed_d.cpu().numpy().view(U32), want_seed, hex)
    if case.unsorted:
        return out
    bits_d = put(np.full((b.n_out, k), FILL_BITS, U32), np.int32)
    rows_d = put(np.full((b.n_out, k), FILL_ROW, np.int64), np.int64)
    scatter_d = put(b.scatter, np.int64) if b.scatter is not None else None
    qn_d = put(b.qn, np.float32) if b.qn is not None else None
    cond, cnt_d = None, None
    if b.cond:
        cnt_d = put(np.array([b.cond[0]], np.int32), np.int32)
        cond = ctypes.byref(RmuCond(cnt_d.data_ptr(), b.cond[1], b.cond[2], b.cond[3]))
    torch.cuda.synchronize()
    rc = fns["final"](lists_d.data_ptr(), parts, nq, k, case.row_base, int(case.l2), qn_d.data_ptr() if qn_d is not None else None,
                      bits_d.data_ptr(), rows_d.data_ptr(), scatter_d.data_ptr() if scatter_d is not None else None, cond, None)
    torch.cuda.synchronize()
    want_bits, want_rows = ref_final(b.lists, k, row_base=case.row_base, l2_out=case.l2, qn=b.qn, scatter=b.scatter, n_out=b.n_out, cond=b.cond)
    if rc != 0:
        out.append(f"final: rc = {rc}")
    out += _first_diff("final: scores (bit patterns)", bits_d.cpu().numpy().view(U32), want_bits, hex)
    out += _first_diff("final: rows", rows_d.cpu().numpy(), want_rows)
    return out
