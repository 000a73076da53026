"""The gathered exact scan (`scan_subset_kernel`, `scan_groups_kernel`: ragmeup_amd/csrc/scan_subset.hip) restated: its two planners, the
row lists that make position and row id differ everywhere, and the GPU cases that hold both kernels to the fmaf chain of
tests/exact_regimes.py bit for bit in every geometry.

A plain helper module, not a fixture: tests/test_subset_regimes_cpu.py reads every constant below back out of the source, proves the
properties of every list a case uses from the restated plan alone, and checks that the cases reach every (width, configuration, tile
class), both block-map branches, one and two query tiles, every nq / k boundary, both group classes, a table with null descriptors and
a Pcap-bound call; tests/test_subset_regimes_gpu.py runs them.

The reference is exact_regimes': the gathered scan runs the MFMA chain of scan_topk.hip, so a (query, row) score is `E.chain` over the
same images.  A list is ascending and the keys carry list positions, so "score descending, position ascending" IS "score descending,
row ascending": the answer of a list is E.expected_topk(chain scores, alive = the row is in the list and not removed, k[, qn2]).
`expected` below ranks the list's columns of the family's chain scores and maps positions back to row ids -- the same answer without
sorting the rows outside the list (the CPU file checks the two against each other).
"""
from __future__ import annotations

import zlib
from dataclasses import dataclass
from functools import lru_cache

import numpy as np

from tests import exact_regimes as E

# ---- constants of scan_subset.hip (tests/test_subset_regimes_cpu.py reads them back; those of scan_common.h / rmu_common.h are E's) -----
K_SPLIT = 32                       # kv = k <= 32 ? 0 : 1
NQ_W1 = 32                         # wq = (nq <= 32 && kv == 0) ? 1 : 4
S_RING = 3                         # SCfg: ScanGeom<D, WQ, CKF, 3, CAP, NCHECK>
# (wq, kv) -> (CKF, CAP, NCHECK): S_w1_k0, S_w4_k0, S_w4_k1
S_CFG = {(1, 0): (48, 64, 1), (4, 0): (96, 64, 1), (4, 1): (32, 128, 2)}
S_W4_K0_CKF_192 = 32               # S_w4_k0: D == 192 ? 32 : 96
IDS_BYTES = 4 * 512                # LDS_BYTES = IDS_OFF + 4 * 512, IDS_OFF = TAIL_OFF
IDS_ROUND = 128                    # rmu_subset_ids_len: (n_sub + 127) / 128 * 128 + 128
XCDS = 8                           # rmu_groups_plan: the deal over 8 XCDs, the table is 8 * longest long
WORK_WAVE = 256                    # tpw = work > 256 ? (work + 255) / 256 : 1
PCAP_SLOTS, PCAP_MAX, PCAP_MIN = 1 << 25, 1024, 4       # pcap = clamp(2^25 / (nq k), 4, 1024)
MAX_QUERIES = 8192                 # kMaxQueriesPerLaunch: the most queries of one grouped call

NQ_MAX = E.NQ_MAX
CONFIGS = ("S_w1_k0", "S_w4_k0", "S_w4_k1")
PIN_QUERIES = (32, 64)             # the queries of the k-order test: 32 of the batch that are aimed at rows, not at flood clusters
NULL_DESC = (0, 0, 0, 0, 0, 0)


def ids_len(n_sub: int) -> int:
    """rmu_subset_ids_len: whole 128-entry tiles and one more of padding"""
    return (n_sub + IDS_ROUND - 1) // IDS_ROUND * IDS_ROUND + IDS_ROUND


def lds_bytes(wq: int, kv: int, dpad: int) -> int:
    ckf, cap, _ = S_CFG[(wq, kv)]
    if (wq, kv) == (4, 0) and dpad == 192:
        ckf = S_W4_K0_CKF_192
    rt = 32 * (4 // wq)
    return S_RING * rt * ckf * 4 + 4 * 32 * cap * 8 + E.LDS_CNT + E.LDS_THR + E.LDS_TRASH + IDS_BYTES


def subset_plan(n_sub: int, nq: int, k: int, dpad: int) -> dict:
    """rmu_subset_plan and the SCfg table"""
    assert 1 <= k <= E.MAX_K and nq >= 1 and n_sub >= 0 and dpad in E.WIDTHS
    kv = 0 if k <= K_SPLIT else 1
    wq = 1 if (nq <= NQ_W1 and kv == 0) else 4
    rp = 4 // wq
    rt = 32 * rp
    nqt = (nq + 32 * wq - 1) // (32 * wq)
    tiles_total = (n_sub + rt - 1) // rt
    s_chunks, tpc = E.plan_chunks(nqt, tiles_total)
    _, cap, ncheck = S_CFG[(wq, kv)]
    return dict(kv=kv, wq=wq, RT=rt, nqt=nqt, tiles_total=tiles_total, s_chunks=s_chunks, tiles_per_chunk=tpc, grid=s_chunks * nqt,
                parts=s_chunks * rp, tiles_last_chunk=tiles_total - (s_chunks - 1) * tpc, xcd_branch=(s_chunks & E.XCD_MASK) == 0,
                lds_bytes=lds_bytes(wq, kv, dpad), CAP=cap, A=32 // ncheck, config=f"S_w{wq}_k{kv}", tile_class=min(tpc, 4),
                ids_len=ids_len(n_sub))


def groups_plan(dpad: int, k: int, list_lengths, q_list) -> dict:
    """rmu_groups_plan.  q_list: the list of each query, non-decreasing.  -> work, tpw, pcap, parts, ids_total, q_off, the groups (class,
    query tiles, tiles, chunks c, tiles per chunk tpc, ids_off), per class the table of (ids_off, t0, ntiles, q_first, q_end, part0) with
    NULL_DESC in the gaps and the LDS bytes, and what FlatIndex.last_geometry() shows behind the call: launches = classes present, grid
    and LDS bytes of the last class launched."""
    assert 1 <= k <= E.MAX_K and dpad in E.WIDTHS
    q_list = [int(v) for v in q_list]
    nq = len(q_list)
    assert 1 <= nq <= MAX_QUERIES and all(a <= b for a, b in zip(q_list, q_list[1:]))
    kv = 0 if k <= K_SPLIT else 1
    groups, q_off, ids_total, work = [], [0] * nq, 0, 0
    q0 = 0
    while q0 < nq:
        q1 = q0 + 1
        while q1 < nq and q_list[q1] == q_list[q0]:
            q1 += 1
        ln = int(list_lengths[q_list[q0]])
        if ln > 0:
            cnt = q1 - q0
            cls = 0 if (cnt <= NQ_W1 and kv == 0) else 1
            wq = 4 if cls else 1
            rt = 32 * (4 // wq)
            g = dict(q0=q0, cnt=cnt, cls=cls, wq=wq, RT=rt, RP=4 // wq, nqt=(cnt + 32 * wq - 1) // (32 * wq), tiles=(ln + rt - 1) // rt,
                     ids_off=ids_total, list=q_list[q0], len=ln)
            ids_total += ids_len(ln)
            assert ids_total < 1 << 32
            q_off[q0:q1] = [g["ids_off"]] * cnt
            work += g["tiles"] * g["nqt"]
            groups.append(g)
        q0 = q1
    tpw = (work + WORK_WAVE - 1) // WORK_WAVE if work > WORK_WAVE else 1
    pcap = min(PCAP_MAX, max(PCAP_MIN, PCAP_SLOTS // (nq * k)))
    parts = 1
    per_xcd = {0: [[] for _ in range(XCDS)], 1: [[] for _ in range(XCDS)]}
    for g in groups:
        c = (g["tiles"] + tpw - 1) // tpw
        g["pcap_bound"] = c > pcap // g["RP"]
        c = min(c, pcap // g["RP"])
        tpc = (g["tiles"] + c - 1) // c
        c = (g["tiles"] + tpc - 1) // tpc                         # (no empty trailing chunk)
        g["c"], g["tpc"] = c, tpc
        parts = max(parts, c * g["RP"])
        for ch in range(c):
            counts = [len(v) for v in per_xcd[g["cls"]]]
            xcd = counts.index(min(counts))                       # the first of the XCDs with the fewest workgroups so far
            t0 = ch * tpc
            t1 = min(t0 + tpc, g["tiles"])
            for qt in range(g["nqt"]):
                per_xcd[g["cls"]][xcd].append((g["ids_off"], t0, t1 - t0, g["q0"] + qt * 32 * g["wq"], g["q0"] + g["cnt"], ch * g["RP"]))
    tab, lds = {}, {}
    for cls in (0, 1):
        longest = max(len(v) for v in per_xcd[cls])
        t = [NULL_DESC] * (longest * XCDS)
        for x in range(XCDS):
            for m, d in enumerate(per_xcd[cls][x]):
                t[m * XCDS + x] = d
        tab[cls] = t
        lds[cls] = lds_bytes(4 if cls else 1, kv if cls else 0, dpad)
    present = [cls for cls in (0, 1) if tab[cls]]
    return dict(work=work, tpw=tpw, pcap=pcap, parts=parts, ids_total=ids_total, q_off=q_off, groups=groups, tab=tab, lds_bytes=lds,
                classes=present, launches=len(present), grid=len(tab[present[-1]]) if present else 0,
                last_lds_bytes=lds[present[-1]] if present else 0,
                nulls={cls: sum(1 for d in tab[cls] if d == NULL_DESC) for cls in (0, 1)})


# ---- the lists --------------------------------------------------------------------------------------------------------------------------
N_ROWS = {192: E.rows_max(192), 384: E.rows_max(384), 768: 72_000}     # rows of a width's index: 768 holds what its longest list needs
SKIP = 3                           # no list names rows 0..2: position p holds a row id >= p + 3
FLOOD_MIN = 4096                   # lists from this length on hold the flood; shorter ones (up to one tile) hold two copies of a few clusters
AIM = 16                           # the cluster whose copies are placed across a chunk boundary: flood_layout()[16], the 384-row "run"
BEFORE = 100                       # ... with this many list positions ahead of the boundary


def held_copies(rows: np.ndarray) -> np.ndarray:
    """The copies of a flood cluster a list holds: never the lowest id, and not every seventh of the rest -- some, but not all, in runs
    that filler does not interrupt.  Of 384 copies 328 stay, of 192 164: more than CAP + 1 for both slot depths (128, 64)."""
    i = np.arange(rows.size)
    keep = (i > 0) & ((i % 7 != 3) | (rows.size < 8))
    return rows[keep]


def span_of(length: int, dpad: int) -> int:
    """the rows a list of this length is sampled from: half as many again, at least the flood, at most the index"""
    return min(N_ROWS[dpad], max(E.FLOOD_END, length + length // 2))


@lru_cache(maxsize=None)
def make_list(length: int, span: int, chunk: int) -> np.ndarray:
    """A strictly ascending int64 list of `length` row ids below `span`, seeded by its arguments.  chunk = the list positions one
    workgroup of the plan it is built for scans (RT * tiles per chunk): the held copies of cluster AIM start BEFORE positions ahead of
    a multiple of it."""
    rng = np.random.default_rng(zlib.crc32(f"subset-list-{length}-{span}-{chunk}".encode()))
    lay = E.flood_layout()
    cluster_rows = np.concatenate([r for _, _, r in lay])
    pool = np.setdiff1d(np.arange(SKIP, span), cluster_rows)
    if length < FLOOD_MIN:
        take = min(8, length // 4)
        held = np.concatenate([r[1:3] for _, _, r in lay[:take]]) if take else np.empty(0, np.int64)
        out = np.sort(np.concatenate([held, rng.choice(pool, length - held.size, replace=False)])).astype(np.int64)
        out.setflags(write=False)
        return out
    assert span >= E.FLOOD_END
    held = np.sort(np.concatenate([held_copies(r) for _, _, r in lay]))
    filler = length - held.size
    r0 = int(held_copies(lay[AIM][2])[0])
    below = pool[pool < r0]
    f0 = int(round(filler * below.size / pool.size))
    fixed = int((held < r0).sum())
    f0 -= (fixed + f0 - (chunk - BEFORE)) % chunk                 # (fixed + f0) = chunk - BEFORE (mod chunk)
    assert 0 <= f0 <= below.size and 0 <= filler - f0 <= pool.size - below.size
    out = np.sort(np.concatenate([held, rng.choice(below, f0, replace=False), rng.choice(pool[pool >= r0], filler - f0, replace=False)])).astype(np.int64)
    out.setflags(write=False)                                     # (cached: shared by every case that names it)
    return out


def class_lengths(rt: int, nqt: int = 1) -> dict:
    """name -> list length for RT rows per tile and nqt query tiles: below one tile, exactly one tile, s RT exactly (one tile per
    workgroup, the XCD-mapped block map; s = the chunks rmu_plan_chunks gives many tiles: 256 with one query tile, 128 with two), the
    smallest lengths with 2, 3 and 4 tiles per workgroup (one live entry in the last tile) and the 3-tile length with L = RT - 1 mod RT"""
    s = E.plan_chunks(nqt, 1 << 20)[0]
    out = {"sub": 20, "one": rt, "t1_xcd": s * rt, "t2": (s + 1) * rt + 1, "t3": (2 * s + 1) * rt + 1, "t3_full": (2 * s + 1) * rt + rt - 1}
    if rt == 32:
        out["t4"] = (3 * s + 1) * rt + 1
    return out


# (nq, k) of every configuration with ONE query tile, from both sides of nq 32|33 at k <= 32, k 32|33 at nq <= 32, with k = 1 and k = 112
# and nq = 128 (the last of one query tile) ...
SHAPES = {
    "S_w1_k0": ((1, 1), (1, 32), (32, 1), (32, 32)),
    "S_w4_k0": ((33, 1), (33, 32), (128, 32)),
    "S_w4_k1": ((1, 33), (32, 33), (33, 33), (128, 112)),
}
# ... and with TWO query tiles: nq = 129 on the other side of 128|129, and 256 with k = 33
SHAPES_NQT2 = {"S_w4_k0": ((129, 32),), "S_w4_k1": ((129, 112), (256, 33))}
NQT2_CLASSES = ("t1_xcd", "t2", "t3")


@dataclass(frozen=True)
class Case:
    dim: int
    corpus: str
    metric: str
    length: int
    nq: int
    k: int
    tag: str = ""

    @property
    def dpad(self) -> int:
        return E.L2_DIMS[self.dim] if self.metric == "l2" else E.DIMS[self.dim]

    @property
    def plan(self) -> dict:
        return subset_plan(self.length, self.nq, self.k, self.dpad)

    @property
    def n(self) -> int:
        """the rows the reference needs: the span the list is sampled from"""
        return span_of(self.length, self.dpad)

    @property
    def rows(self) -> np.ndarray:
        p = self.plan
        return make_list(self.length, self.n, p["RT"] * p["tiles_per_chunk"])

    @property
    def id(self) -> str:
        return f"{self.metric}-{self.corpus}-d{self.dim}-L{self.length}-nq{self.nq}-k{self.k}" + (f"-{self.tag}" if self.tag else "")


def _rt(config: str) -> int:
    return 128 if config == "S_w1_k0" else 32


def _grid(dim: int) -> list:
    out = []
    for config in CONFIGS:
        for name, length in class_lengths(_rt(config)).items():
            out += [Case(dim, "random", "ip", length, nq, k, name) for nq, k in SHAPES[config]]
        for name in NQT2_CLASSES:
            out += [Case(dim, "random", "ip", class_lengths(32, 2)[name], nq, k, name + "_nqt2") for nq, k in SHAPES_NQT2.get(config, ())]
    return out


def _monotone(dim: int) -> list:
    """rising / falling at the deepest tile class of each geometry, k in {1, 32, 33, 112}"""
    out = []
    for kind in ("rising", "falling"):
        out += [Case(dim, kind, "ip", class_lengths(128)["t3"], 32, k, "t3") for k in (1, 32)]
        out += [Case(dim, kind, "ip", class_lengths(32)["t4"], 128, k, "t4") for k in (1, 32, 33, 112)]
        out += [Case(dim, kind, "ip", class_lengths(32)["t4"], 32, k, "t4") for k in (33, 112)]
    return out


def _metric_cases(metric: str, dim: int) -> list:
    """one case per geometry, each with at least 2 tiles per workgroup"""
    return [Case(dim, "scaled", metric, class_lengths(128)["t2"], 32, 32, "t2"), Case(dim, "scaled", metric, class_lengths(32)["t3"], 128, 32, "t3"),
            Case(dim, "scaled", metric, class_lengths(32)["t4"], 33, 33, "t4")]


CASES = ([c for d in E.DIMS for c in _grid(d)] + [c for d in E.DIMS for c in _monotone(d)]
         + [c for d in (100, 384, 768) for c in _metric_cases("cosine", d)] + [c for d in E.L2_DIMS for c in _metric_cases("l2", d)])


def families(cases=None) -> dict:
    """(dim, corpus, metric) -> its cases: ONE index and ONE pass of the chain serve a family"""
    out = {}
    for c in (CASES if cases is None else cases):
        out.setdefault((c.dim, c.corpus, c.metric), []).append(c)
    return {f: sorted(v, key=lambda c: (c.length, c.nq, c.k)) for f, v in out.items()}


# ---- the reference of a family --------------------------------------------------------------------------------------------------------
class Reference(E.Reference):
    """E.Reference (the chain scores of a family, one pass per query bucket) with the answer of a LIST: the list's columns ranked,
    positions mapped back to row ids."""

    def __init__(self, dim: int, kind: str, metric: str, cases):
        super().__init__(dim, kind, metric, cases)
        self._last = (None, None)                              # the ranked list of the last (pass, list, mask): the cases of a list are adjacent

    def expected(self, rows, nq: int, k: int, alive=None, row_base: int = 0, queries=None) -> tuple:
        """rows: the list as the kernel sees it (int64; entries outside [0, n) are absent; n = the rows of the chain pass, which is
        the whole index wherever a test places absent ids).  alive: bool per LIST POSITION, or None.  queries: indices into the family's
        batch (default: its first nq)."""
        rows = np.asarray(rows, np.int64)
        b = NQ_MAX if queries is not None else min(v for v in self.scores if v >= nq)       # the smallest pass of the chain that holds them
        n = self.scores[b].shape[1]
        ok = (rows >= 0) & (rows < n)
        if alive is not None:
            ok &= np.asarray(alive, bool)
        key = (b, rows.tobytes(), ok.tobytes(), row_base)
        if key != self._last[0]:
            if rows.size:
                rs, rp = E.ranked(self.scores[b][:, np.where(ok, rows, 0)], ok, E.MAX_K)
                rr = np.where(rp >= 0, rows[np.maximum(rp, 0)] + row_base, -1)
            else:
                rs, rr = np.empty((b, 0), np.float32), np.empty((b, 0), np.int64)
            self._last = (key, (rs, rr))
        rs, rr = self._last[1]
        sel = np.arange(nq) if queries is None else np.asarray(queries, np.int64)
        return E.topk_from_order(rs[sel], rr[sel], k, None if self.qn2 is None else self.qn2[sel])



def geometry_mismatch(g: dict, grid: int, lds: int, launches: int) -> str:
    if (g["grid"], g["lds_bytes"], g["launches"]) != (grid, lds, launches):
        return f"ran {g}, planned grid {grid} with {lds} LDS bytes in {launches} launch(es)"
    return ""


def run_family(flat_index, family, cases, ref=None) -> tuple:
    """One index of the family's (dim, metric) with every row of its longest span; every case must run the planned geometry
    (FlatIndex.last_geometry: grid, LDS bytes, one launch) and return the reference's bits and rows.  -> (failures, cases checked)"""
    dim, kind, metric = family
    ref = ref or Reference(dim, kind, metric, cases)
    idx = flat_index(dim, metric=E._METRIC[metric])
    idx.add(ref.x[:ref.n_max])
    failures = []
    for c in cases:
        p = c.plan
        s, r = idx.search(ref.q[:c.nq], c.k, rows=c.rows)
        what = f"{c.id} [{p['config']}, {p['tiles_per_chunk']} tiles per workgroup, {p['nqt']} query tiles]"
        g = geometry_mismatch(idx.last_geometry(), p["grid"], p["lds_bytes"], 1)
        if g:
            failures.append(f"{what}: {g}")
        m = E.mismatch(s, r, *ref.expected(c.rows, c.nq, c.k))
        if m:
            failures.append(f"{what}: {m}")
    idx.close()
    return failures, len(cases)


# ---- the grouped calls ------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class GroupCall:
    """One rmu_index_search_groups call over the `random` corpus of `dim`: lists (row-id arrays) in list order, and per group, in query
    order, (list number, the indices of its queries in the family's batch)."""
    name: str
    dim: int
    k: int
    lists: tuple
    groups: tuple

    @property
    def q_list(self) -> np.ndarray:
        return np.concatenate([np.full(len(qi), li, np.int64) for li, qi in self.groups])

    @property
    def q_index(self) -> np.ndarray:
        return np.concatenate([np.asarray(qi, np.int64) for _, qi in self.groups])

    @property
    def plan(self) -> dict:
        return groups_plan(E.DIMS[self.dim], self.k, [len(v) for v in self.lists], self.q_list)

    @property
    def n(self) -> int:
        return max([int(v[-1]) + 1 for v in self.lists if len(v)] + [E.FLOOD_END])


def _lst(length: int, dpad: int, chunk: int) -> np.ndarray:
    return make_list(length, span_of(length, dpad), chunk)


def _empty() -> np.ndarray:
    return np.empty(0, np.int64)


@lru_cache(maxsize=None)
def group_calls(dim: int = 384) -> tuple:
    dpad = E.DIMS[dim]
    a = np.arange
    out = []
    # one group, 3 tiles per workgroup: class 0 (1 query, k <= 32, 65 665 rows: W = 514), class 1 at k <= 32 (33 queries) and at k > 32
    out.append(GroupCall("one_group_w1_tpw3", dim, 32, (_lst(class_lengths(128)["t3"], dpad, 384),), ((0, a(16, 17)),)))
    out.append(GroupCall("one_group_w4_k0_tpw3", dim, 32, (_lst(class_lengths(32)["t3"], dpad, 96),), ((0, a(0, 33)),)))
    out.append(GroupCall("one_group_w4_k1_tpw3", dim, 33, (_lst(class_lengths(32)["t3"], dpad, 96),), ((0, a(16, 17)),)))
    # mixed: groups of 33, 1, 5 (on an EMPTY list), 129, 31, 128 and 32 queries; list 4 is used by nobody; lists 6 and 7 overlap (7 is a
    # slice of 6).  The groups start at queries 0, 33, 34, 39, 168, 199, 327: inside a 32-lane fragment all but the first
    l6 = _lst(3001, dpad, 32)
    lists = (_lst(2003, dpad, 32), _lst(20_011, dpad, 128), _empty(), _lst(4001, dpad, 32), _lst(777, dpad, 32), _lst(5003, dpad, 128),
             l6, np.ascontiguousarray(l6[500:1601]))
    out.append(GroupCall("mixed", dim, 32, lists, ((0, a(0, 33)), (1, a(33, 34)), (2, a(34, 39)), (3, a(39, 168)), (5, a(168, 199)),
                                                   (6, a(100, 228)), (7, a(0, 32)))))
    # Pcap bites: nq = 8192, k = 112: pcap = 36.  8063 queries on a 1-row list (work 63), 129 on a 6400-row list (200 tiles x 2 query
    # tiles): W = 463, tpw = 2, and the big group is cut into 34 chunks of 6 tiles (c_g = pcap / RP = 36, then the second rounding), not 100 of 2
    out.append(GroupCall("pcap", dim, 112, (np.array([4321], np.int64), _lst(6400, dpad, 192)),
                         ((0, a(8063) % NQ_MAX), (1, a(129)))))
    # the flood lists of family 1 inside a grouped call, one group per class, the queries aimed at the clusters
    out.append(GroupCall("flood", dim, 32, (_lst(class_lengths(128)["t2"], dpad, 256), _lst(class_lengths(32)["t3"], dpad, 96)),
                         ((0, a(0, 24)), (1, np.concatenate([a(0, 24), a(40, 80)])))))
    out.append(GroupCall("flood_k112", dim, 112, (_lst(class_lengths(32)["t4"], dpad, 128), _lst(class_lengths(32)["t2"], dpad, 64)),
                         ((0, a(0, 24)), (1, a(0, 130)))))
    return tuple(out)


def run_group_call(idx, ref, call: GroupCall, device_lists: bool = False) -> list:
    """-> failures: the planned geometry (launches = classes present, grid and LDS bytes of the last class) and, per query, the chain
    reference of ITS list"""
    p = call.plan
    lists = list(call.lists)
    if device_lists:
        import torch
        lists = [torch.from_numpy(np.array(v)).cuda() for v in lists]
    qi = call.q_index
    s, r = idx.search_groups(ref.q[qi], call.k, lists, call.q_list)
    failures = []
    g = geometry_mismatch(idx.last_geometry(), p["grid"], p["last_lds_bytes"], p["launches"])
    if g:
        failures.append(f"{call.name}: {g}")
    at = 0
    for li, q in call.groups:
        es, er = ref.expected(call.lists[li], len(q), call.k, queries=q)
        m = E.mismatch(s[at:at + len(q)], r[at:at + len(q)], es, er)
        if m:
            failures.append(f"{call.name}: group of {len(q)} queries from query {at} on list {li} ({len(call.lists[li])} rows): {m}")
        at += len(q)
    return failures
