"""The exact fp32 scan (`scan_topk_kernel`, ragmeup_amd/csrc/scan_topk.hip) restated: its planner, its arithmetic as an fmaf chain in the
kernel's own k order, the image kernels that prepare COSINE and L2 rows and queries, the merge's last L2 step, the order of the answer --
and the inputs and GPU cases that hold the kernel to that restatement bit for bit in every geometry.

A plain helper module, not a fixture: tests/test_exact_regimes_cpu.py reads every constant below back out of the source, checks the
planner's invariants, that CASES reaches every configuration, tile class, block-map branch and boundary, that the C chain and the numpy
chain agree, and that every corpus has the property it is built for; tests/test_exact_regimes_gpu.py runs CASES.

The contract (scan_topk.hip's header): v_mfma_f32_32x32x2_f32 is exact fp32, "== a k-ordered fmaf chain", and the k-permutation fixes
the order: for step t of dpad / 8, for MFMA c of 4, first k = 8t + c, then k = 8t + 4 + c.  A score is therefore ONE bit pattern, whatever
the configuration, the tile a row falls in or the batch a query travels with, and the answer is its k best (score descending, row
ascending) with no tolerance and no tie rule.
"""
from __future__ import annotations

import zlib
from dataclasses import dataclass
from fractions import Fraction
from functools import lru_cache

import numpy as np

from oracle import cflat

# ---- constants of scan_topk.hip / scan_common.h / rmu_common.h (tests/test_exact_regimes_cpu.py reads them back) -------------------------
K_SPLIT = 32                       # kv = k <= 32 ? 0 : 1
MAX_K = 112                        # RMU_MAX_K
NQ_W1, NQ_W2 = 32, 64              # wq = nq <= 32 ? 1 : (nq <= 64 ? 2 : 4)
PROMOTED_WQ = 2                    # kv == 1 && wq == 1 -> wq = 2
WIDTHS = (192, 384, 768)           # the padded widths the kernel is built for
# (wq, kv) -> (CKF, RING, CAP, NCHECK): the Cfg table
CFG = {(4, 0): (96, 4, 64, 1), (4, 1): (96, 2, 128, 2), (2, 0): (96, 3, 64, 1), (2, 1): (48, 2, 128, 2), (1, 0): (48, 3, 64, 1)}
CHUNKS_FIRST, CHUNKS_LAST, CHUNKS_STEP = 8, 256, 8       # rmu_plan_chunks: for (s = 8; s <= 256; s += 8)
CU_ROUND = 256                     # ... eff = total / roundup(total, 256); stop at total >= 256 && eff > 0.999
XCD_MASK = 7                       # block_map: (s_chunks & 7) == 0 -> the XCD-mapped branch
LDS_CNT, LDS_THR, LDS_TRASH, LDS_GT = 4 * 32 * 4, 4 * 32 * 4, 256 * 8, 4 * 256     # ScanGeom / Cfg: counts, thresholds, trash, shared-threshold landing zone
DEEP_K, DEEP_N = 32, 262_144       # k > 32 && n >= 262144: the deep ladder takes over (out of scope here)

CONFIGS = ("w1_k0", "w1_k0_nt", "w2_k0", "w2_k0_nt", "w2_k1", "w4_k0", "w4_k1")


def plan_chunks(nqt: int, tiles_total: int) -> tuple:
    """rmu_plan_chunks: (s_chunks, tiles_per_chunk)"""
    best_s, best_eff = CHUNKS_FIRST, -1.0
    for s in range(CHUNKS_FIRST, CHUNKS_LAST + 1, CHUNKS_STEP):
        total = s * nqt
        eff = float(total) / float(((total + CU_ROUND - 1) // CU_ROUND) * CU_ROUND)
        if eff > best_eff + 1e-9:
            best_eff, best_s = eff, s
        if total >= CU_ROUND and eff > 0.999:
            break
    s = best_s
    if tiles_total < s:
        s = tiles_total if tiles_total > 0 else 1
    tpc = max((tiles_total + s - 1) // s, 1)
    used = (tiles_total + tpc - 1) // tpc
    if 0 < used < s:
        s = used
    return s, tpc


def plan(n: int, nq: int, k: int, dpad: int, nt_env: int = 1) -> dict:
    """rmu_scan_plan for the register-resident scan.  nt_env: RMU_NT (default 1)."""
    assert 1 <= k <= MAX_K and nq >= 1 and n >= 0 and dpad in WIDTHS
    kv = 0 if k <= K_SPLIT else 1
    wq = 1 if nq <= NQ_W1 else (2 if nq <= NQ_W2 else 4)
    if kv == 1 and wq == 1:
        wq = PROMOTED_WQ
    rp = 4 // wq
    rt = 32 * rp
    nqt = (nq + 32 * wq - 1) // (32 * wq)
    tiles_total = (n + rt - 1) // rt
    s_chunks, tpc = plan_chunks(nqt, tiles_total)
    nt = 1 if (nt_env and nqt == 1 and kv == 0 and wq <= 2) else 0
    ckf, ring, cap, ncheck = CFG[(wq, kv)]
    lds = ring * rt * ckf * 4 + 4 * 32 * cap * 8 + LDS_CNT + LDS_THR + LDS_TRASH + LDS_GT
    last = tiles_total - (s_chunks - 1) * tpc
    return dict(kv=kv, wq=wq, nt=nt, RT=rt, nqt=nqt, tiles_total=tiles_total, s_chunks=s_chunks, tiles_per_chunk=tpc, grid=s_chunks * nqt,
                parts=s_chunks * rp, tiles_last_chunk=last, xcd_branch=(s_chunks & XCD_MASK) == 0, lds_bytes=lds, CAP=cap, A=32 // ncheck,
                config=f"w{wq}_k{kv}" + ("_nt" if nt else ""), tile_class=min(tpc, 4))


# ---- the arithmetic ---------------------------------------------------------------------------------------------------------------------
def pad(a, dpad: int) -> np.ndarray:
    a = np.ascontiguousarray(a, dtype=np.float32)
    if a.shape[1] == dpad:
        return a
    out = np.zeros((a.shape[0], dpad), np.float32)
    out[:, :a.shape[1]] = a
    return out


def k_order(dpad: int) -> np.ndarray:
    """the columns in the order the MFMA chain adds them"""
    return np.array([8 * t + 4 * h + c for t in range(dpad // 8) for c in range(4) for h in range(2)], np.int64)


def _round_f32(v: Fraction) -> np.float32:
    """v -> fp32, round to nearest even, normal range"""
    if v == 0:
        return np.float32(0.0)
    a = abs(v)
    e = a.numerator.bit_length() - a.denominator.bit_length()
    if Fraction(2) ** e > a:
        e -= 1
    assert Fraction(2) ** e <= a < Fraction(2) ** (e + 1) and -126 <= e <= 127
    m = a / Fraction(2) ** (e - 23)
    lo = m.numerator // m.denominator
    rest = m - lo
    if rest > Fraction(1, 2) or (rest == Fraction(1, 2) and (lo & 1)):
        lo += 1
    r = np.float32(float(Fraction(lo) * Fraction(2) ** (e - 23)))          # 24 (25 after a carry: a power of two) bits: exact in both formats
    return -r if v < 0 else r


def chain_numpy(q, x, dpad: int, track=None) -> np.ndarray:
    """The chain without fmaf: the fp64 product of two fp32 numbers is exact, so fp64(acc) + product is ONE rounding short of fmaf's --
    it double-rounds only when the fp64 sum sits exactly on an fp32 midpoint (low 29 bits of the pattern == 1 << 28); those elements are
    redone with exact rationals.  `track` (a dict) receives the smallest non-zero |product| and |partial sum| met."""
    q, x = pad(q, dpad).astype(np.float64), pad(x, dpad).astype(np.float64)
    acc = np.zeros((q.shape[0], x.shape[0]), np.float32)
    tiny_p = tiny_s = np.inf
    for kk in k_order(dpad):
        prod = q[:, kk, None] * x[None, :, kk]
        s = acc.astype(np.float64) + prod
        new = s.astype(np.float32)
        mid = (s.view(np.uint64) & np.uint64((1 << 29) - 1)) == np.uint64(1 << 28)
        for i, j in zip(*np.nonzero(mid)):
            new[i, j] = _round_f32(Fraction(float(acc[i, j])) + Fraction(float(q[i, kk])) * Fraction(float(x[j, kk])))
        acc = new
        if track is not None:
            nzp, nzs = np.abs(prod[prod != 0]), np.abs(acc[acc != 0])
            tiny_p = min(tiny_p, float(nzp.min(initial=np.inf)))
            tiny_s = min(tiny_s, float(nzs.min(initial=np.inf)))
    if track is not None:
        track["product"], track["sum"] = tiny_p, tiny_s
    return acc


def chain(q, x, dpad: int) -> np.ndarray:
    """[nq, n] fp32: oracle_chain_scores (oracle/flat_search.c)"""
    return cflat.chain_scores(q, x, dpad)


# ---- the image kernels of rmu_api.hip and the merge's last L2 step, restated from their comments --------------------------------------------
_TINY = np.float32(1e-12)


def row_norm_image(v, dpad: int) -> np.ndarray:
    """k_row_norm (COSINE rows and queries): s = the wave's |row|^2 over dpad columns, inv = 1 / max(sqrt(s), 1e-12), row *= inv"""
    v = pad(v, dpad)
    s = cflat.wave_sumsq(v, dpad)
    inv = np.float32(1.0) / np.maximum(np.sqrt(s, dtype=np.float32), _TINY)
    return (v * inv[:, None]).astype(np.float32)


def l2_rows_image(v, dim: int, dpad: int) -> np.ndarray:
    """k_l2_aug_rows: column `dim` <- -|row|^2 summed over `dim` columns"""
    v = pad(v, dpad).copy()
    v[:, dim] = -cflat.wave_sumsq(v, dim)
    return v


def l2_queries_image(v, dim: int, dpad: int) -> tuple:
    """k_l2_aug_queries: (the stored query (2q, 1), |q|^2)"""
    v = pad(v, dpad).copy()
    qn2 = cflat.wave_sumsq(v, dim)
    v *= np.float32(2.0)
    v[:, dim] = np.float32(1.0)
    return v, qn2


def l2_merge(qn2, s) -> np.ndarray:
    """rmu_merge_final_launch with l2_out: score = max(|q|^2 - s, 0), one fp32 subtraction"""
    return np.maximum(qn2[:, None].astype(np.float32) - s.astype(np.float32), np.float32(0.0)).astype(np.float32)


def images(metric: str, q, x, dim: int, dpad: int) -> tuple:
    """(stored queries, stored rows, |q|^2 or None) of an index of this metric"""
    if metric == "ip":
        return pad(q, dpad), pad(x, dpad), None
    if metric == "cosine":
        return row_norm_image(q, dpad), row_norm_image(x, dpad), None
    qi, qn2 = l2_queries_image(q, dim, dpad)
    return qi, l2_rows_image(x, dim, dpad), qn2


def expected_topk(scores, alive, k: int, qn2=None) -> tuple:
    """The answer: (score descending, row ascending) over the live, non-NaN rows, padded with (-inf, -1); -0.0 is +0.0 as in the key
    (prev + 0.0f).  qn2: an L2 index -- ranked by the scan's score, reported as max(|q|^2 - s, 0), padded with (+inf, -1)."""
    return topk_from_order(*ranked(scores, alive, k), k, qn2)


def ranked(scores, alive, depth: int) -> tuple:
    """(scores, rows) of the `depth` best per query; a stable sort of the negated scores orders equal scores by row"""
    s = np.asarray(scores, np.float32) + np.float32(0.0)
    dead = np.isnan(s)
    if alive is not None:
        dead |= ~np.asarray(alive, bool)[None, :]
    s = np.where(dead, np.float32(-np.inf), s)
    nq, n = s.shape
    depth = min(depth, n)
    # candidates: everything >= the depth-th best value (all its ties included), then the stable sort
    out_s = np.full((nq, depth), -np.inf, np.float32)
    out_r = np.full((nq, depth), -1, np.int64)
    kth = np.partition(s, n - depth, axis=1)[:, n - depth]
    for i in range(nq):
        cand = np.nonzero((s[i] >= kth[i]) & ~dead[i])[0]
        order = cand[np.argsort(-s[i, cand], kind="stable")][:depth]
        out_s[i, :order.size] = s[i, order]
        out_r[i, :order.size] = order
    return out_s, out_r


def topk_from_order(rs, rr, k: int, qn2=None) -> tuple:
    nq = rs.shape[0]
    out_s = np.full((nq, k), -np.inf, np.float32)
    out_r = np.full((nq, k), -1, np.int64)
    kk = min(k, rs.shape[1])
    out_s[:, :kk], out_r[:, :kk] = rs[:, :kk], rr[:, :kk]
    if qn2 is not None:
        out_s = np.where(out_r >= 0, l2_merge(qn2, out_s), np.float32(np.inf)).astype(np.float32)
    return out_s, out_r


def bits(a) -> np.ndarray:
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- the corpora ------------------------------------------------------------------------------------------------------------------------
DIMS = {100: 192, 384: 384, 767: 768, 768: 768}          # dim -> dpad of an IP / COSINE index
L2_DIMS = {100: 192, 383: 384, 767: 768}                 # an L2 index pads dim + 1
NQ_MAX = 256
UNIT = 384                       # flood placements are laid out in 384-row units: at the 3-tile row counts a unit is 1 / 2 / 4 whole chunks
FLOOD_SIZES = (384, 192, 129, 113, 65, 34, 33, 2)      # 3 CAP and CAP + 1 of both depths (CAP 128, 64), k + 1 for k = 112, 33, 32, 1
ZERO_QUERY = 24                  # position of the all-zero query in every batch that is long enough


def rows_max(dpad: int) -> int:
    """the 3- and 4-tile classes of RT = 128 run at dpad 192 and 384 only"""
    return 768 * 128 + 129 if dpad < 768 else 768 * 64 + 65


def _unit(v):
    v = np.asarray(v, np.float32)
    return np.ascontiguousarray(v / np.linalg.norm(v.astype(np.float64), axis=1, keepdims=True).astype(np.float32), dtype=np.float32)


def flood_layout(sizes: tuple = FLOOD_SIZES) -> list:
    """[(m, placement, rows)]: query i of every batch is aimed at cluster i.  "spread": a few copies (fewer than any k > 7) at the END of
    one unit -- the last rows its workgroup scans -- and the rest over the next two units: the k lowest ids come from several
    workgroups, and the one that holds the lowest meets a shared bound EQUAL to their score.  "boundary": a contiguous run centred on
    row 128 of a unit, a tile boundary inside a chunk for every RT.  "run": a contiguous run from the start of a tile.
    `sizes`: the cluster sizes (tests/wide_regimes.py has its own, for the slot depths of the wide scan)."""
    out, c = [], 1
    for m in sizes:
        a = max(1, min(7, m // 3))
        b = (m - a + 1) // 2
        rows = np.concatenate([UNIT * (c + 1) - a + np.arange(a), UNIT * (c + 1) + 17 + np.arange(b), UNIT * (c + 2) + 1 + 2 * np.arange(m - a - b)])
        out.append((m, "spread", rows.astype(np.int64)))
        c += 3
    for m in sizes:
        if m // 2 > 128:
            c += 1
        out.append((m, "boundary", (UNIT * c + 128 - m // 2 + np.arange(m)).astype(np.int64)))
        c += 2 if m > 256 else 1
    second = False
    for m in sizes:                        # (two to a unit where they fit: at row 0, and at row 256 -- the start of a tile for every RT)
        if second and m > UNIT - 256:
            c, second = c + 1, False
        out.append((m, "run", (UNIT * c + (256 if second else 0) + np.arange(m)).astype(np.int64)))
        if second or m > 256:
            c, second = c + 1, False
        else:
            second = True
    return out


FLOOD_END = 16_000               # every cluster lies below this row: present at each 3-tile row count (16 417 the smallest)


@lru_cache(maxsize=2)
def corpus(kind: str, dim: int, n: int = 0, sizes: tuple = FLOOD_SIZES) -> tuple:
    """(x [n, dim], q [NQ_MAX, dim]) fp32, seeded; n = 0: rows_max of the width.  The rows of a smaller n are the first rows of a larger one
    (`falling` excepted) and the queries do not depend on n.  `sizes`: the flood clusters, as in flood_layout; any dim with an explicit n.
    random   unit rows with the flood clusters written over them; queries 0..23 aimed at the clusters (unit(v + 0.3 unit noise)), query 24
             all zero, the rest next to rows below 4000 (present at every row count of CASES)
    rising   rows c_r u, c_r = 1 + r / 65536, queries unit(u + 0.5 unit noise): u.q > 0 and every row beats all lower rows
    falling  the same rows in reverse order
    scaled   `random` with rows of norm 0.25 .. 4 and queries of norm 0.5 .. 2 (COSINE and L2 cases: the image kernels have work to do)"""
    n = n or rows_max(DIMS.get(dim) or L2_DIMS[dim])
    rng_x, rng, rng_s = (np.random.default_rng(zlib.crc32(f"exact-{kind}-{dim}-{what}".encode())) for what in ("rows", "queries", "scales"))
    if kind in ("random", "scaled"):
        x = _unit(rng_x.standard_normal((n, dim), dtype=np.float32))
        q = np.empty((NQ_MAX, dim), np.float32)
        lay = flood_layout(sizes)
        for i, (m, _, rows) in enumerate(lay):
            v = _unit(rng.standard_normal((1, dim), dtype=np.float32))
            x[rows[rows < n]] = v
            q[i] = _unit(v + np.float32(0.3) * _unit(rng.standard_normal((1, dim), dtype=np.float32)))[0]
        assert n >= 4000
        free = np.setdiff1d(np.arange(4000), np.concatenate([r for _, _, r in lay]))
        near = rng.choice(free, NQ_MAX - len(lay), replace=False)
        q[len(lay):] = _unit(x[near] + np.float32(0.3) * _unit(rng.standard_normal((near.size, dim), dtype=np.float32)))
        q[ZERO_QUERY] = 0.0
        if kind == "scaled":
            rep = np.arange(n)
            for _, _, rows in lay:
                rep[rows[rows < n]] = rows[0]                         # the copies of a cluster stay bit-identical
            x = np.ascontiguousarray(x * rng_s.uniform(0.25, 4.0, (n, 1)).astype(np.float32)[rep])
            q = np.ascontiguousarray(q * rng.uniform(0.5, 2.0, (NQ_MAX, 1)).astype(np.float32))
        return x, q
    if kind not in ("rising", "falling"):
        raise ValueError(kind)
    u = _unit(rng.standard_normal((1, dim), dtype=np.float32))
    c = (np.float32(1.0) + np.arange(n, dtype=np.float32) / np.float32(65536.0)).astype(np.float32)
    x = np.ascontiguousarray(c[:, None] * u, dtype=np.float32)
    q = _unit(u + np.float32(0.5) * _unit(rng.standard_normal((NQ_MAX, dim), dtype=np.float32)))
    return (np.ascontiguousarray(x[::-1]) if kind == "falling" else x), q


# ---- the cases --------------------------------------------------------------------------------------------------------------------------
def class_rows(rt: int) -> dict:
    """name -> n for a configuration with RT rows per tile and ONE query tile: the smallest row counts with 2, 3 and 4 tiles per workgroup
    (each with one live row in the last tile), 256 RT exactly (one tile each, the XCD-mapped block map, n = 0 mod RT) and a 3-tile count
    with n = RT - 1 mod RT"""
    return {"t1_xcd": 256 * rt, "t2": 257 * rt + 1, "t3": 513 * rt + 1, "t4": 769 * rt + 1, "t3_full": 513 * rt + rt - 1}


# (nq, k) of every configuration, from both sides of nq 32|33, 64|65, 128|129 and k 32|33, with k = 1 and k = 112
SHAPES = {
    128: ((1, 1), (1, 32), (32, 1), (32, 32)),                                                 # w1_k0(_nt)
    64: ((33, 1), (33, 32), (64, 32), (1, 33), (32, 33), (32, 112), (33, 33), (64, 112)),      # w2_k0(_nt), w2_k1 (promoted from nq <= 32, and its own)
    32: ((65, 1), (65, 32), (128, 32), (65, 33), (128, 112), (129, 32), (129, 112)),           # w4_k0, w4_k1, one and two query tiles
}


@dataclass(frozen=True)
class Case:
    dim: int
    corpus: str
    metric: str
    n: int
    nq: int
    k: int
    tag: str = ""

    @property
    def dpad(self) -> int:
        return L2_DIMS[self.dim] if self.metric == "l2" else DIMS[self.dim]

    @property
    def plan(self) -> dict:
        return plan(self.n, self.nq, self.k, self.dpad)

    @property
    def id(self) -> str:
        return f"{self.metric}-{self.corpus}-d{self.dim}-n{self.n}-nq{self.nq}-k{self.k}" + (f"-{self.tag}" if self.tag else "")


def _grid(dim: int) -> list:
    dpad = DIMS[dim]
    out = []
    for rt, shapes in SHAPES.items():
        for name, n in class_rows(rt).items():
            if n > rows_max(dpad):
                continue
            out += [Case(dim, "random", "ip", n, nq, k, name) for nq, k in shapes]
    # two query tiles in the XCD-mapped branch (128 chunks) with one tile per workgroup
    # (8192 rows, among the row counts above, give 129 queries 256 tiles: 2 per workgroup)
    out += [Case(dim, "random", "ip", 4096, 256, 33, "nqt2_xcd")]
    return out


def _monotone(dim: int) -> list:
    """rising / falling at k in {1, 32, 33, 112}, at the deepest tile class of each RT"""
    dpad = DIMS[dim]
    out = []
    for kind in ("rising", "falling"):
        for rt, nqs in ((128, (32,)), (64, (64, 32)), (32, (128, 129))):
            n = max(v for v in class_rows(rt).values() if v <= rows_max(dpad))
            for nq in nqs:
                for k in (1, 32, 33, 112):
                    if plan(n, nq, k, dpad)["RT"] == rt:
                        out.append(Case(dim, kind, "ip", n, nq, k, f"rt{rt}"))
    return out


def _metric_cases(metric: str, dim: int) -> list:
    """one case per tile class >= 2: w4_k0 with 2 and with 4 tiles, w2_k1 with 3"""
    return [Case(dim, "scaled", metric, class_rows(32)["t2"], 65, 32, "t2"), Case(dim, "scaled", metric, class_rows(32)["t4"], 65, 32, "t4"),
            Case(dim, "scaled", metric, class_rows(64)["t3"], 33, 33, "t3")]


CASES = ([c for d in DIMS for c in _grid(d)] + [c for d in DIMS for c in _monotone(d)]
         + [c for d in (100, 384, 768) for c in _metric_cases("cosine", d)] + [c for d in L2_DIMS for c in _metric_cases("l2", d)])


def families(cases=None) -> dict:
    """(dim, corpus, metric) -> its cases in ascending n: ONE index, grown by `add`, serves a family"""
    out = {}
    for c in (CASES if cases is None else cases):
        out.setdefault((c.dim, c.corpus, c.metric), []).append(c)
    return {f: sorted(v, key=lambda c: (c.n, c.nq, c.k)) for f, v in out.items()}


# the reduced grid of the environment-switched forms (RMU_NT=0: the plain w1_k0 / w2_k0; RMU_NO_SHARED_THR=1: share_thr = 0):
# every (width, w1_k0 | w2_k0) with 2 and 3 tiles per workgroup -- the `random` corpus carries the flood -- and the rising corpus
def variant_cases() -> list:
    out = []
    for dim in DIMS:
        dpad = DIMS[dim]
        for rt, (nq, k) in ((128, (32, 32)), (64, (64, 32))):
            for name in ("t2", "t3"):
                n = class_rows(rt)[name]
                if n <= rows_max(dpad):
                    out.append(Case(dim, "random", "ip", n, nq, k, name))
    for rt, nq in ((128, 32), (64, 64), (64, 32), (32, 128)):
        for k in (32, 112):
            if plan(class_rows(rt)["t3"], nq, k, 384)["RT"] == rt:
                out.append(Case(384, "rising", "ip", class_rows(rt)["t3"], nq, k, f"rt{rt}"))
    return out


# ---- the reference of a family, computed once -------------------------------------------------------------------------------------------
class Reference:
    """Chain scores of a family (dim, corpus, metric): per RT class the queries that class can use against the rows it needs, the
    ranked lists per (RT class, n) -- all from ONE pass of the chain per RT class."""

    def __init__(self, dim: int, kind: str, metric: str, cases):
        self.dim, self.kind, self.metric = dim, kind, metric
        self.dpad = L2_DIMS[dim] if metric == "l2" else DIMS[dim]
        need = {}                                             # nq bucket -> rows
        for c in cases:
            b = self._bucket(c.nq)
            need[b] = max(need.get(b, 0), c.n)
        self.n_max = max(need.values())
        self.x, self.q = corpus(kind, dim, self.n_max)
        qi, xi, self.qn2 = images(metric, self.q, self.x[:self.n_max], dim, self.dpad)
        self.scores = {b: chain(qi[:b], xi[:n], self.dpad) for b, n in need.items()}
        self._ranked = {}

    @staticmethod
    def _bucket(nq: int) -> int:
        return 32 if nq <= 32 else (64 if nq <= 64 else NQ_MAX)

    def topk(self, n: int, nq: int, k: int, alive=None) -> tuple:
        b = self._bucket(nq)
        key = (b, n, None if alive is None else alive.tobytes())
        if key not in self._ranked:
            self._ranked[key] = ranked(self.scores[b][:, :n], None if alive is None else alive[:n], MAX_K)
        rs, rr = self._ranked[key]
        return topk_from_order(rs[:nq], rr[:nq], k, None if self.qn2 is None else self.qn2[:nq])


def holes(p: dict, n: int, top1) -> np.ndarray:
    """rows to delete at a geometry: the first and the last row of a tile, a whole tile, a whole chunk, the best row of every query"""
    rt, tpc = p["RT"], p["tiles_per_chunk"]
    chunk = rt * tpc
    rows = [np.array([5 * rt, 6 * rt - 1]), 9 * rt + np.arange(rt), 3 * chunk + np.arange(chunk), np.asarray(top1, np.int64)]
    r = np.unique(np.concatenate(rows))
    return r[r < n]


def mismatch(got_s, got_r, exp_s, exp_r) -> str:
    """"" when the answers are the same bits, else the first difference"""
    gs, es = bits(got_s), bits(exp_s)
    gr, er = np.asarray(got_r, np.int64), np.asarray(exp_r, np.int64)
    bad = np.nonzero((gs != es) | (gr != er))
    if bad[0].size == 0:
        return ""
    i, j = int(bad[0][0]), int(bad[1][0])
    return (f"{bad[0].size} of {gs.size} entries differ; first at query {i} rank {j}: got (0x{gs[i, j]:08x}, row {gr[i, j]}), "
            f"expected (0x{es[i, j]:08x}, row {er[i, j]})")


# ---- the runner the GPU file and tests/exact_variant_driver.py share ----------------------------------------------------------------------
_METRIC = {"ip": 0, "cosine": 1, "l2": 2}                  # RMU_METRIC_IP / COSINE / L2SQ


def run_family(flat_index, family, cases, nt_env: int = 1, ref=None) -> tuple:
    """One index of the family's (dim, metric), grown by `add` through the ascending n of its cases; every case must run the planned
    regime (FlatIndex.last_geometry: grid, LDS bytes, one launch) and return the reference's bits.  -> (failures, cases checked)"""
    dim, kind, metric = family
    ref = ref or Reference(dim, kind, metric, cases)
    idx = flat_index(dim, metric=_METRIC[metric])
    idx.set_screening(False)
    failures, have = [], 0
    for c in sorted(cases, key=lambda c: (c.n, c.nq, c.k)):
        if c.n > have:
            idx.add(ref.x[have:c.n])
            have = c.n
        p = plan(c.n, c.nq, c.k, c.dpad, nt_env)
        s, r = idx.search(ref.q[:c.nq], c.k)
        g = idx.last_geometry()
        what = f"{c.id} [{p['config']}, {p['tiles_per_chunk']} tiles per workgroup, {p['nqt']} query tiles]"
        if (g["grid"], g["lds_bytes"], g["launches"]) != (p["grid"], p["lds_bytes"], 1):
            failures.append(f"{what}: ran {g}, planned grid {p['grid']} with {p['lds_bytes']} LDS bytes in one launch")
        m = mismatch(s, r, *ref.topk(c.n, c.nq, c.k))
        if m:
            failures.append(f"{what}: {m}")
    idx.close()
    return failures, len(cases)
