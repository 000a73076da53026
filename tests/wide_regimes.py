"""The wide exact scan (`scan_wide_kernel`, ragmeup_amd/csrc/scan_wide.hip: rows of 769..3072 dimensions and every RMU_OPT_WIDE_SCAN search)
restated: its planner and the inputs and GPU cases that hold it to the fmaf chain of tests/exact_regimes.py, bit for bit, in every geometry.

A plain helper module, not a fixture, in the style of tests/exact_regimes.py, from which everything that does not depend on the width is
imported: the chain and its numpy twin, the image kernel of COSINE rows, the order of the answer, rmu_plan_chunks, the rows to delete.
tests/test_wide_regimes_cpu.py reads every constant below back out of the source, checks the planner's invariants, that the cases reach
every configuration, tile class, block-map branch, query-tile count and boundary, and that every corpus has the property it is built for;
tests/test_wide_regimes_gpu.py runs the cases.

The contract (scan_wide.hip's header): the k-permutation and the one accumulator chain per (row, query) are scan_topk_kernel's, so "a score
has the bits scan_topk_kernel gives it, whatever the batch, k, geometry or row range" -- ONE bit pattern per (query, row), the chain's,
and the answer is its k best (score descending, row ascending) with no tolerance and no tie rule.  What the wide kernel has of its own:
the queries are streamed through the ring beside the rows (a run-time chunk loop of dpad / CKF steps), the threshold filter runs at the
end of a tile, and k > 32 keeps 64 x 64 tiles whatever the batch, with a slot depth no other kernel has (CAP 120, a check every four rows).
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np

from tests import exact_regimes as E
from tests.exact_regimes import (bits, chain, chain_numpy, expected_topk, holes, k_order, mismatch, pad, plan_chunks, ranked,  # noqa: F401
                                 row_norm_image, topk_from_order)

# ---- constants of scan_wide.hip / rmu_api.hip / rmu.h (tests/test_wide_regimes_cpu.py reads them back) -----------------------------------
K_SPLIT = 32                       # kv = k <= 32 ? 0 : 1
MAX_K = 112                        # RMU_MAX_K
NQ_W1, NQ_W2 = 32, 64              # kv == 0: wq = nq <= 32 ? 1 : (nq <= 64 ? 2 : 4)
KV1_WQ = 2                         # kv == 1: wq = 2 whatever the batch
MAX_DIM, MAX_DIM_WIDE = 768, 3072  # RMU_MAX_DIM, RMU_MAX_DIM_WIDE
PAD_TO = 64                        # pad_dim above 768: (d + 63) / 64 * 64
DPAD_MIN, DPAD_STEP = 64, 32       # rmu_wide_plan accepts 64 <= dpad <= RMU_MAX_DIM_WIDE, dpad % 32 == 0
# (wq, kv) -> (CKF, RING, CAP, NCHECK): the WCfg table
WCFG = {(4, 0): (32, 3, 64, 1), (2, 0): (32, 3, 64, 1), (1, 0): (32, 3, 64, 1), (2, 1): (16, 3, 120, 4)}
LDS_CNT, LDS_THR, LDS_TRASH, LDS_GT = 4 * 32 * 4, 4 * 32 * 4, 256 * 8, 4 * 256     # counts, thresholds, trash, shared-threshold landing zone
LDS_LIMIT = 160 * 1024
XCD_MASK = E.XCD_MASK              # block_map is scan_common.h's
DEEP_K, DEEP_N = E.DEEP_K, E.DEEP_N
DEEP_FIRST, DEEP_RATIO, DEEP_ALIGN, DEEP_LEVELS = 8192, 4, 128, 8       # deep_bounds: RMU_DEEP_FIRST, RMU_DEEP_RATIO, whole 128-row units, at most 8 levels

CONFIGS = ("w1_k0_nt", "w2_k0_nt", "w4_k0", "w2_k1")          # the default process
PLAIN_CONFIGS = ("w1_k0", "w2_k0")                            # RMU_NT=0 only


def pad_dim(d: int) -> int:
    """pad_dim of rmu_api.hip (IP / COSINE)"""
    if d <= MAX_DIM:
        return 192 if d <= 192 else (384 if d <= 384 else 768)
    return (d + PAD_TO - 1) // PAD_TO * PAD_TO if d <= MAX_DIM_WIDE else -1


def plan_wide(n: int, nq: int, k: int, dpad: int, nt_env: int = 1) -> dict:
    """rmu_wide_plan.  nt_env: RMU_NT (default 1)."""
    assert 1 <= k <= MAX_K and nq >= 1 and n >= 0 and DPAD_MIN <= dpad <= MAX_DIM_WIDE and dpad % DPAD_STEP == 0
    kv = 0 if k <= K_SPLIT else 1
    wq = KV1_WQ if kv == 1 else (1 if nq <= NQ_W1 else (2 if nq <= NQ_W2 else 4))
    rp = 4 // wq
    rt = 32 * rp
    nqt = (nq + 32 * wq - 1) // (32 * wq)
    tiles_total = (n + rt - 1) // rt
    s_chunks, tpc = plan_chunks(nqt, tiles_total)
    nt = 1 if (nt_env and nqt == 1 and kv == 0 and wq <= 2) else 0
    ckf, ring, cap, ncheck = WCFG[(wq, kv)]
    lds = ring * (rt + 32 * wq) * ckf * 4 + 4 * 32 * cap * 8 + LDS_CNT + LDS_THR + LDS_TRASH + LDS_GT
    last = tiles_total - (s_chunks - 1) * tpc
    return dict(kv=kv, wq=wq, nt=nt, RT=rt, nqt=nqt, tiles_total=tiles_total, s_chunks=s_chunks, tiles_per_chunk=tpc, grid=s_chunks * nqt,
                parts=s_chunks * rp, tiles_last_chunk=last, xcd_branch=(s_chunks & XCD_MASK) == 0, lds_bytes=lds, CAP=cap, A=32 // ncheck,
                CKF=ckf, nch=dpad // ckf, config=f"w{wq}_k{kv}" + ("_nt" if nt else ""), tile_class=min(tpc, 4))


def deep_bounds(n: int) -> list:
    """deep_bounds of rmu_api.hip with the default RMU_DEEP_FIRST / RMU_DEEP_RATIO: the row counts the ladder's levels end at"""
    b = [n]
    c = n // DEEP_RATIO // DEEP_ALIGN * DEEP_ALIGN
    while c >= DEEP_FIRST and len(b) < DEEP_LEVELS:
        b.insert(0, c)
        c = c // DEEP_RATIO // DEEP_ALIGN * DEEP_ALIGN
    return b


# ---- the corpora ------------------------------------------------------------------------------------------------------------------------
# 769: the smallest dpad; 1000 / 1024: the same dpad with and without padding columns (dim == dpad takes the other branch of the row copy in
# rmu_index_add and lets device queries be read in place); 3072: the longest chunk loop (nch 96 / 192); 832: nch 26 / 52, no powers of two
WIDE_DIMS = {769: 832, 1000: 1024, 1024: 1024, 1536: 1536, 3072: 3072}
# 3 CAP and CAP + 1 of both wide slot depths (CAP 64: 192, 65; CAP 120: 384 >= 360, 121), k + 1 for k = 112, 33, 32, 1.  (E.FLOOD_SIZES with
# 121 in the place of 129: as many clusters, so E.ZERO_QUERY and the 384-row unit layout carry over and every cluster lies below E.FLOOD_END)
FLOOD_SIZES = (384, 192, 121, 113, 65, 34, 33, 2)
NQ_MAX, UNIT, ZERO_QUERY, FLOOD_END = E.NQ_MAX, E.UNIT, E.ZERO_QUERY, E.FLOOD_END
CORPUS_BYTES = 512 << 20           # no family's rows take more


def dpad_of(dim: int) -> int:
    return WIDE_DIMS.get(dim) or E.DIMS[dim]


def flood_layout() -> list:
    return E.flood_layout(FLOOD_SIZES)


def rows_max(dpad: int) -> int:
    """the 3-tile counts of RT = 128 run where their rows fit CORPUS_BYTES"""
    return 513 * 128 + 127 if (513 * 128 + 127) * dpad * 4 <= CORPUS_BYTES else 257 * 128 + 1


def corpus(kind: str, dim: int, n: int) -> tuple:
    """exact_regimes.corpus at a wide width, with the wide flood clusters (a narrow width: that module's own corpus, unchanged)"""
    return E.corpus(kind, dim, n, FLOOD_SIZES) if dim in WIDE_DIMS else E.corpus(kind, dim, n)


# ---- the cases --------------------------------------------------------------------------------------------------------------------------
def class_rows(rt: int) -> dict:
    """name -> n for a configuration with RT rows per tile and ONE query tile: 256 RT exactly (one tile each, the XCD-mapped block map, n = 0
    mod RT), the smallest row counts with 2 and 3 tiles per workgroup (one live row in the last tile; three tiles: the prologue, the steady
    ring and the clamped tail reloads of issue_chunk), a 3-tile count with n = RT - 1 mod RT, and the small counts of the other block-map
    branch and the short chunks"""
    return {"t1_xcd": 256 * rt, "t2": 257 * rt + 1, "t3": 513 * rt + 1, "t3_full": 513 * rt + rt - 1, "one": 1, "few": 31, "t1_small": 5 * rt + 3}


# (nq, k) of every configuration, from both sides of nq 32|33 and 64|65 and k 32|33, with k = 1 and k = 112; w2_k1 has 1, 1, 1, 1, 2, 3 and 4
# query tiles of 64 -- a regime the narrow scan does not have
SHAPES = {
    128: ((1, 1), (1, 32), (32, 1), (32, 32)),                                                            # w1_k0(_nt)
    64: ((33, 1), (33, 32), (64, 32)) + tuple((nq, k) for k in (33, 112) for nq in (1, 32, 33, 64, 65, 129, 256)),     # w2_k0(_nt), w2_k1
    32: ((65, 1), (65, 32), (128, 32), (129, 32), (256, 32)),                                             # w4_k0, one and two query tiles
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
        return dpad_of(self.dim)

    @property
    def plan(self) -> dict:
        return plan_wide(self.n, self.nq, self.k, self.dpad)

    @property
    def id(self) -> str:
        return f"{self.metric}-{self.corpus}-d{self.dim}-n{self.n}-nq{self.nq}-k{self.k}" + (f"-{self.tag}" if self.tag else "")


def _grid(dim: int, names=None) -> list:
    """`names`: RT -> the row counts of class_rows to run (default: all)"""
    out = []
    for rt, shapes in SHAPES.items():
        for name, n in class_rows(rt).items():
            if names is None or name in names[rt]:
                out += [Case(dim, "random", "ip", n, nq, k, name) for nq, k in shapes]
    return out


_BIG = {128: ("t2",), 64: ("t2",), 32: ("t2", "t3")}       # 1536 and 3072 dimensions: every configuration with 2 tiles, RT = 32 with 3 as well


def _monotone(dim: int) -> list:
    """rising / falling at k in {1, 32, 33, 112}, at the deepest tile class of each RT that fits"""
    out = []
    for kind in ("rising", "falling"):
        for rt, nqs in ((128, (32,)), (64, (64, 32)), (32, (128,))):
            n = max(v for v in class_rows(rt).values() if v <= rows_max(dpad_of(dim)))
            for nq in nqs:
                for k in (1, 32, 33, 112):
                    if plan_wide(n, nq, k, dpad_of(dim))["RT"] == rt:
                        out.append(Case(dim, kind, "ip", n, nq, k, f"rt{rt}"))
    return out


def _cosine(dim: int) -> list:
    """w4_k0 with 2 and with 3 tiles, w2_k1 with 3"""
    return [Case(dim, "scaled", "cosine", class_rows(32)["t2"], 65, 32, "t2"), Case(dim, "scaled", "cosine", class_rows(32)["t3"], 65, 32, "t3"),
            Case(dim, "scaled", "cosine", class_rows(64)["t3"], 33, 33, "t3")]


CASES = (_grid(769) + _grid(1024) + _grid(1536, _BIG) + _grid(3072, _BIG)
         + [Case(1000, "scaled", "cosine", class_rows(32)["t2"], 65, 32, "t2"), Case(1000, "scaled", "cosine", class_rows(64)["t3"], 33, 33, "t3"),
            Case(1000, "random", "ip", class_rows(64)["t2"], 33, 32, "t2")]
         + _monotone(769) + _monotone(3072) + _cosine(769) + _cosine(1024) + _cosine(1536))

# the narrow corpora, built to break a selection, through the wide kernel (RMU_OPT_WIDE_SCAN; nch = 6..48): the 2- and 3-tile cases of every
# RT of exact_regimes' random / IP families at 100 and 768 dimensions and of scaled / COSINE at 384, planned by plan_wide and held to the
# references exact_regimes.Reference computes for scan_topk_kernel -- both kernels are tied to one reference, not to each other
NARROW_CASES = [Case(c.dim, c.corpus, c.metric, c.n, c.nq, c.k, c.tag) for c in E.CASES
                if (c.dim, c.corpus, c.metric) in ((100, "random", "ip"), (768, "random", "ip"), (384, "scaled", "cosine")) and c.tag in ("t2", "t3")]


def families(cases=None) -> dict:
    """(dim, corpus, metric) -> its cases in ascending n: ONE index, grown by `add`, serves a family"""
    out = {}
    for c in (CASES + NARROW_CASES if cases is None else cases):
        out.setdefault((c.dim, c.corpus, c.metric), []).append(c)
    return {f: sorted(v, key=lambda c: (c.n, c.nq, c.k)) for f, v in out.items()}


# the reduced grid of the environment-switched forms (RMU_NT=0: the plain w1_k0 / w2_k0, which nothing else reaches; RMU_NO_SHARED_THR=1:
# share_thr = 0): the smallest and the largest width x {w1_k0, w2_k0} with 2 and 3 tiles per workgroup over the `random` corpus, which
# carries the flood, and the rising corpus at 769 dimensions for every RT at k = 32 and k = 112
def variant_cases() -> list:
    out = []
    for dim in (769, 3072):
        for rt, (nq, k) in ((128, (32, 32)), (64, (64, 32))):
            for name in ("t2", "t3"):
                n = class_rows(rt)[name]
                if n <= rows_max(dpad_of(dim)):
                    out.append(Case(dim, "random", "ip", n, nq, k, name))
    for rt, nq, k in ((128, 32, 32), (64, 64, 32), (32, 128, 32), (64, 32, 112), (64, 128, 112)):
        out.append(Case(769, "rising", "ip", class_rows(rt)["t3"], nq, k, f"rt{rt}"))
    return out


# ---- the reference of a family, computed once -------------------------------------------------------------------------------------------
class Reference(E.Reference):
    """exact_regimes.Reference at a wide width (IP and COSINE: there is no wide L2 index).  The buckets are by query count alone -- k > 32
    sends every batch through 64-row tiles -- so each bucket's chain covers the most rows any of its cases needs."""

    def __init__(self, dim: int, kind: str, metric: str, cases):
        assert metric in ("ip", "cosine")
        self.dim, self.kind, self.metric = dim, kind, metric
        self.dpad = dpad_of(dim)
        need = {}                                             # nq bucket -> rows
        for c in cases:
            b = self._bucket(c.nq)
            need[b] = max(need.get(b, 0), c.n)
        self.n_max = max(max(need.values()), 4000)            # (the `random` corpus aims its last queries at rows below 4000)
        self.x, self.q = corpus(kind, dim, self.n_max)
        qi, xi, self.qn2 = E.images(metric, self.q, self.x, dim, self.dpad)
        self.scores = {b: chain(qi[:b], xi[:n], self.dpad) for b, n in need.items()}
        self._ranked = {}


def reference(dim: int, kind: str, metric: str, cases):
    return Reference(dim, kind, metric, cases) if dim in WIDE_DIMS else E.Reference(dim, kind, metric, cases)


# ---- the runner the GPU file and tests/wide_variant_driver.py share ---------------------------------------------------------------------
def geometry_mismatch(g: dict, p: dict) -> str:
    """"" when FlatIndex.last_geometry() reports the planned regime in one launch"""
    if (g["grid"], g["lds_bytes"], g["launches"]) == (p["grid"], p["lds_bytes"], 1):
        return ""
    return f"ran {g}, planned grid {p['grid']} with {p['lds_bytes']} LDS bytes in one launch"


def run_family(flat_index, family, cases, nt_env: int = 1, ref=None) -> tuple:
    """One index of the family's (dim, metric), grown by `add` through the ascending n of its cases (a narrow width: with RMU_OPT_WIDE_SCAN);
    every case must run the planned regime (FlatIndex.last_geometry: grid, LDS bytes, one launch) and return the reference's bits.
    -> (failures, cases checked)"""
    dim, kind, metric = family
    ref = ref or reference(dim, kind, metric, cases)
    idx = flat_index(dim, metric=E._METRIC[metric])
    idx.set_screening(False)
    if dim not in WIDE_DIMS:
        idx.set_wide_scan(True)
    failures, have = [], 0
    for c in sorted(cases, key=lambda c: (c.n, c.nq, c.k)):
        if c.n > have:
            idx.add(ref.x[have:c.n])
            have = c.n
        assert c.n == have, "a family's cases run in ascending n"
        p = plan_wide(c.n, c.nq, c.k, c.dpad, nt_env)
        s, r = idx.search(ref.q[:c.nq], c.k)
        what = f"{c.id} [{p['config']}, {p['tiles_per_chunk']} tiles per workgroup, {p['nqt']} query tiles, {p['nch']} chunks per tile]"
        g = geometry_mismatch(idx.last_geometry(), p)
        if g:
            failures.append(f"{what}: {g}")
        m = mismatch(s, r, *ref.topk(c.n, c.nq, c.k))
        if m:
            failures.append(f"{what}: {m}")
    idx.close()
    return failures, len(cases)


# ---- the threshold ladder (k > 32 over >= 262 144 rows: every level a launch of the wide kernel with a row0 and seeded shared thresholds) --
LADDER_DIM, LADDER_N, LADDER_NQ = 769, 262_144 + 77, 8
LADDER_FLOODS = ((113, 16_384), (34, 65_536))       # (copies, centre): k + 1 for k = 112 and 33, across the first two level ends
LADDER_LATE = (7, 240, 100)                         # a third flood inside the last level: (lowest copies, the others, chunk of the lowest)


def ladder_floods() -> list:
    """rows of each flood.  The first two lie across a level's end.  The third is "spread" inside the last level, at that launch's own
    geometry: 7 copies in the LAST rows of one workgroup's chunk, 240 (two slot depths) in the first tiles of the chunk after the next --
    that workgroup fills its slots, compacts and publishes the copies' score as the shared bound long before the first one reaches its
    last tile, whose 7 copies (the lowest rows: they belong to every answer) then meet a bound EQUAL to their score."""
    out = [centre - m // 2 + np.arange(m) for m, centre in LADDER_FLOODS]
    start = deep_bounds(LADDER_N)[-2]
    p = plan_wide(LADDER_N - start, LADDER_NQ, MAX_K, WIDE_DIMS[LADDER_DIM])
    chunk = p["RT"] * p["tiles_per_chunk"]
    few, rest, c0 = LADDER_LATE
    return out + [np.concatenate([start + chunk * (c0 + 1) - few + np.arange(few), start + chunk * (c0 + 2) + 17 + np.arange(rest)])]


def ladder_corpus() -> tuple:
    """(x, q, [rows of each flood]): unit-norm Gaussian rows; flood i is the best of query i, bit-identical copies on both sides of a level's
    end -- the level's k-th best then seeds the next level with a bound EQUAL to the scores still to come (the filter passes v >= bound) --
    or spread inside the last level (ladder_floods)"""
    rng = np.random.default_rng(769_262_221)
    x = rng.standard_normal((LADDER_N, LADDER_DIM), dtype=np.float32)
    x /= np.sqrt(np.einsum("ij,ij->i", x, x, dtype=np.float64)).astype(np.float32)[:, None]
    q = E._unit(x[rng.choice(4000, LADDER_NQ, replace=False)] + np.float32(0.3) * E._unit(rng.standard_normal((LADDER_NQ, LADDER_DIM), dtype=np.float32)))
    floods = ladder_floods()
    for i, rows in enumerate(floods):
        v = E._unit(rng.standard_normal((1, LADDER_DIM), dtype=np.float32))
        x[rows] = v
        q[i] = E._unit(v + np.float32(0.3) * E._unit(rng.standard_normal((1, LADDER_DIM), dtype=np.float32)))[0]
    return x, q, floods


# ---- a shared bound EQUAL to the score of rows still to come, inside one launch ---------------------------------------------------------
# The `spread` clusters of the flood corpora put their lowest rows in the last tile of a workgroup with 3 tiles; the workgroup that
# publishes their score as the shared bound compacts at the end of ITS second tile (a wave's slot takes 32 rows per tile and is checked
# at CAP - A = 32), and a bound is fetched one tile ahead of its use: whether the bound arrives first is a race there.  With 5 tiles per
# workgroup it is not: LATE gives every k <= 32 configuration its smallest 5-tile row count, a cluster whose 7 lowest rows end chunk
# LATE_CHUNK and whose other 3 RT rows begin the chunk after the next.  (k > 32 publishes at 112 of 120: ladder_floods, 13 tiles.)
LATE_DIM, LATE_FEW, LATE_CHUNK = 769, 7, 20
LATE = ((32, 65, 32), (64, 64, 32), (128, 32, 32))              # (RT, nq, k): w4_k0, w2_k0_nt, w1_k0_nt


def late_rows(rt: int) -> int:
    return 1025 * rt + 1


def late_floods() -> list:
    out = []
    for rt, nq, k in LATE:
        chunk = rt * plan_wide(late_rows(rt), nq, k, WIDE_DIMS[LATE_DIM])["tiles_per_chunk"]
        out.append(np.concatenate([chunk * (LATE_CHUNK + 1) - LATE_FEW + np.arange(LATE_FEW), chunk * (LATE_CHUNK + 2) + np.arange(3 * rt)]))
    return out


def late_corpus() -> tuple:
    """(x, q, floods): unit-norm Gaussian rows, flood i the best of query i, the other queries next to rows below 4000"""
    n, nq = max(late_rows(rt) for rt, _, _ in LATE), max(nq for _, nq, _ in LATE)
    rng = np.random.default_rng(769_131_201)
    x = rng.standard_normal((n, LATE_DIM), dtype=np.float32)
    x /= np.sqrt(np.einsum("ij,ij->i", x, x, dtype=np.float64)).astype(np.float32)[:, None]
    floods = late_floods()
    free = np.setdiff1d(np.arange(4000), np.concatenate(floods))
    q = E._unit(x[rng.choice(free, nq, replace=False)] + np.float32(0.3) * E._unit(rng.standard_normal((nq, LATE_DIM), dtype=np.float32)))
    for i, rows in enumerate(floods):
        v = E._unit(rng.standard_normal((1, LATE_DIM), dtype=np.float32))
        x[rows] = v
        q[i] = E._unit(v + np.float32(0.3) * E._unit(rng.standard_normal((1, LATE_DIM), dtype=np.float32)))[0]
    return x, q, floods


def chain_blocked(q, x, dpad: int, block: int = 32_768) -> np.ndarray:
    """chain over a corpus too large to pad in one piece"""
    return np.concatenate([chain(q, x[a:a + block], dpad) for a in range(0, x.shape[0], block)], axis=1)
