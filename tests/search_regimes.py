"""The search dispatcher (`rmu_index_search` in ragmeup_amd/csrc/rmu_api.hip) restated in Python, the inputs whose number of
re-run queries is known WITHOUT the library, and the GPU cases that pin every re-run class from both sides of each boundary.

A plain helper module, not a fixture: tests/test_search_regimes_cpu.py reads every constant below back out of the source, checks
that the re-run classes partition the flagged counts and that CASES reaches every class and boundary, and verifies the verdicts
of the small cases on the CPU; tests/test_search_regimes_gpu.py runs CASES against the fp64 oracle.

The verdict of a query (k_rescore, scan_screen.hip):  ok = isfinite(eps) && (nvalid < K' || s~[K'-1] < s~[k-1] - 2 eps),
with |s~ - s_fp32| <= eps and eps <= 1.05 EPS, EPS = eps() of tests/test_screen_bound_cpu.py (test_screen_error_bound_on_hardware).
  certain FAIL  the best row exists >= K' times as bit-identical copies (identical rows -> identical approximate scores, so
                s~[K'-1] == s~[k-1]), and leads every other row by >= 5 EPS so that the copies ARE the first K' candidates;
                or the query overflows fp16 (|64 q_i| > 65504: eps is not finite).
  certain PASS  in fp64 the k-th best live score exceeds the K'-th best by >= 5 EPS:  tau >= s_k - E, smin <= s_K' + E with
                E <= 1.05 EPS; the test passes when s_k - s_K' > 4 E, 4 E <= 4.2 EPS; the rest of the 5 covers fp64 against the
                fp32 chain (2.3e-5 |x||q|, a twentieth of EPS on unit vectors).
A batch built from these two kinds only has an exactly known count: FlatIndex.last_screened() must return minus that count.
"""
from __future__ import annotations

import zlib
from dataclasses import dataclass
from functools import lru_cache

import numpy as np

from oracle import oracle as O

# ---- constants of rmu_api.hip / rmu_common.h (tests/test_search_regimes_cpu.py reads them back) -------------------------------
MAX_QUERIES_PER_LAUNCH = 8192     # kMaxQueriesPerLaunch: a request is cut into blocks of this many queries
ONE_CLASS_MAX_NB = 32             # one_class = nb <= 32: anything flagged re-runs the whole block, no gather
SMALL_N = 32                      # small_n = min(nb, 32): the 32-query geometry of the "small" launch
MID_DIV = 8                       # mid_n = nb / 8
SCREEN_KP = 32                    # kScreenKp: K' for k <= KP_STEP1
KP_STEP1, KP_STEP2, KP_AT_STEP2 = 24, 32, 40       # screen_kp: 32 up to k = 24, 40 up to k = 32, ...
KP_DEEP_DIV, KP_DEEP_MIN = 5, 8                     # ... then k + max(8, k / 5) ...
KS_CAP, KS_CAP_DEEP = 48, 128                       # RMU_KS_CAP, RMU_KS_CAP_DEEP (candidate slots) ...
KP_DEEP_MAX = KS_CAP_DEEP - 8                       # ... capped at RMU_KS_CAP_DEEP - 8 = 120
SCREEN_MAX_K = 104                # kScreenMaxK
PAYS_NB = 128                     # screen_pays: nb >= 128
PAYS_N = 3_000_000                #   || n >= 3000000
PAYS_MID_NB, PAYS_MID_N = 64, 1_000_000             #   || (nb > 64 && n >= 1000000) || a minimum batch was set
DEEP_K, DEEP_N = 32, 262_144      #   || (k > 32 && n >= 262144); deep_applies: k > 32 && n >= 262144
SCREEN_DIM = 384                  # geom: dim == 384 (and the padded row / the norm column that go with it)
XNORM_CAP = 500.0                 # xnorm_max < 500.f: fp16(64 x) must not overflow

MARGIN_EPS = 5.0                  # the verdict rule above, in units of EPS
GRADE_STEP = 4e-6                 # relative step between the copies of a graded cluster (K' + 8 of them stay inside one fp16 cell)
MAX_CLUSTERS = 160                # flagged queries have a duplicate cluster each up to here; beyond, they cycle over these


def screen_kp(k: int) -> int:
    if k <= KP_STEP1:
        return SCREEN_KP
    if k <= KP_STEP2:
        return KP_AT_STEP2
    return min(k + max(KP_DEEP_MIN, k // KP_DEEP_DIV), KP_DEEP_MAX)


def path(n: int, nb: int, k: int, dim: int, metric: str = "ip", screening: bool = True, min_nq: int = 0, xnorm_max: float = 1.0) -> str:
    """Which branch of rmu_index_search answers a block of nb queries: "screen", "deep_ladder" or "exact".  It assumes an index
    that holds the fp16 image (`idx->split`: every index of dim 384 on a default build) with the screening left enabled unless
    `screening` says otherwise.  `metric` is taken for the call sites' sake and does not enter: at dim 384 the inner-product and
    cosine indexes have the 384-wide padded row and the L2 index its norm column."""
    screen_pays = nb >= PAYS_NB or n >= PAYS_N or (nb > PAYS_MID_NB and n >= PAYS_MID_N) or min_nq > 0 or (k > DEEP_K and n >= DEEP_N)
    geom = dim == SCREEN_DIM
    if (screening and geom and nb >= max(min_nq, 1) and screen_pays and k <= SCREEN_MAX_K and n > 0 and 0.0 < xnorm_max < XNORM_CAP):
        return "screen"
    if k > DEEP_K and n >= DEEP_N:
        return "deep_ladder"
    return "exact"


def rerun_class(nb: int, c: int) -> tuple:
    """(class, queries the answering launch is planned for) of a screened block of nb queries of which c were flagged."""
    if c == 0:
        return "none", 0
    if nb <= ONE_CLASS_MAX_NB:
        return "whole_one_class", nb
    mid_n = nb // MID_DIV
    if c > mid_n:
        return "whole", nb
    if mid_n > SMALL_N and c > SMALL_N:
        return "mid", mid_n
    return "small", SMALL_N


def blocks(nq: int) -> list:
    """[(first query, queries)] of the blocks a request of nq queries is cut into."""
    return [(q0, min(MAX_QUERIES_PER_LAUNCH, nq - q0)) for q0 in range(0, nq, MAX_QUERIES_PER_LAUNCH)]


# ---- EPS (tests/test_screen_bound_cpu.py's eps(), with the maxima over the rows taken once per corpus) ---------------------------
def _image(v):
    return (v.astype(np.float32) * np.float32(64.0)).astype(np.float16)


def corpus_maxima(x) -> tuple:
    """(|dx|max, |x|max) over the rows, in slabs (a 270 000-row corpus in fp64 is not held at once)."""
    dx = xn = 0.0
    for lo in range(0, x.shape[0], 32768):
        xd = x[lo:lo + 32768].astype(np.float64)
        dx = max(dx, float(np.linalg.norm(xd - _image(x[lo:lo + 32768]).astype(np.float64) / 64.0, axis=1).max()))
        xn = max(xn, float(np.linalg.norm(xd, axis=1).max()))
    return dx, xn


def eps_numpy(dx: float, xn: float, q, l2: bool = False):
    """eps(x, q) / eps_l2(x, q) of tests/test_screen_bound_cpu.py from the corpus maxima."""
    qd = q.astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        dq = np.linalg.norm(qd - _image(q).astype(np.float64) / 64.0, axis=1)
    qn = np.linalg.norm(qd, axis=1)
    return dx * qn + xn * dq + dx * dq + 5e-5 * xn * qn + (1.5e-5 * xn * xn if l2 else 0.0)


def _unit32(v):
    v = np.asarray(v, np.float32)
    return np.ascontiguousarray(v / np.linalg.norm(v, axis=1, keepdims=True), dtype=np.float32)


# ---- exact fp64 top lists ---------------------------------------------------------------------------------------------------------
_METRIC = {"ip": O.METRIC_IP, "cosine": O.METRIC_COSINE, "l2": O.METRIC_L2SQ}


def oracle_topk(q, x, k: int, metric: str = "ip", alive=None, budget: int = 1 << 25, rep=None):
    """oracle.flat_search for wide batches: the same fp64 scores (oracle.scores_f64) and the same order (-score, row), but the k
    survivors are found by a partition instead of a sort of every row, in query chunks that keep the score matrix small.
    `rep` (optional, one entry per row): rep[i] != i names the row that row i is a bit-identical copy of; the copy then takes that
    row's score.  The fp64 matrix product may sum two identical rows in different orders (they differ by 1e-16 then), which would
    order exact ties by noise instead of by row id and pick an arbitrary k of a cluster."""
    nq, n = q.shape[0], x.shape[0]
    out_s = np.full((nq, k), -np.inf)
    out_r = np.full((nq, k), -1, np.int64)
    step = max(1, min(1024, budget // max(n, 1)))
    for lo in range(0, nq, step):
        s = O.scores_f64(q[lo:lo + step], x, _METRIC[metric])
        if rep is not None:
            copy = np.nonzero(rep != np.arange(n))[0]
            s[:, copy] = s[:, rep[copy]]
        if alive is not None:
            s[:, ~alive] = -np.inf
        kk = min(k, n)
        kth = np.partition(s, n - kk, axis=1)[:, n - kk]
        for i in range(s.shape[0]):
            cand = np.nonzero((s[i] >= kth[i]) & (s[i] > -np.inf))[0]                # every row tied with the k-th included
            order = cand[np.lexsort((cand, -s[i, cand]))][:k]
            out_s[lo + i, :order.size] = s[i, order]
            out_r[lo + i, :order.size] = order
    return out_s, out_r


def _top_lists(q, x, depth: int, metric: str):
    """The `depth` best fp64 scores and rows of every query over a corpus WITHOUT exact duplicates: an fp32 product preselects
    depth + 32 rows, fp64 re-scores them; the guard asserts the preselection cannot have lost one of the `depth`."""
    nq, n = q.shape[0], x.shape[0]
    pre = min(n, depth + 32)
    top_s = np.empty((nq, depth))
    top_r = np.empty((nq, depth), np.int64)
    x2 = (x.astype(np.float32) ** 2).sum(1) if metric == "l2" else None
    step = max(1, min(256, (1 << 27) // n))
    for lo in range(0, nq, step):
        qc = q[lo:lo + step]
        s32 = qc @ x.T
        if metric == "l2":
            s32 = 2.0 * s32 - x2[None, :]
        part = np.argpartition(-s32, pre - 1, axis=1)[:, :pre] if pre < n else np.broadcast_to(np.arange(n), (qc.shape[0], n))
        xg = x[part].astype(np.float64)
        s64 = np.einsum("qcd,qd->qc", xg, qc.astype(np.float64))
        if metric == "l2":
            s64 = -((qc.astype(np.float64) ** 2).sum(1)[:, None] - 2.0 * s64 + (xg * xg).sum(2))
        order = np.lexsort((part, -s64), axis=1)
        s64, part = np.take_along_axis(s64, order, 1), np.take_along_axis(part, order, 1)
        if pre < n:          # the worst preselected row is far enough below the depth-th for fp32 to have ordered them right
            assert (s64[:, depth - 1] - s64[:, pre - 1] > 1e-4 * np.maximum(1.0, np.abs(s64[:, 0]))).all(), "preselection too shallow"
        top_s[lo:lo + step], top_r[lo:lo + step] = s64[:, :depth], part[:, :depth]
    return top_s, top_r


# ---- candidate pools: a base corpus, certain-pass candidates and their fp64 top lists (computed once, shared by the cases) -----------
DEEP_CLUSTERS, DEEP_PER_CLUSTER = 68, 16


def _planted(x, m: int, seed: int):
    """m queries next to corpus rows (oracle.make_queries, in slabs with their own seeds when m exceeds the corpus)."""
    out, left, i = [], m, 0
    while left > 0:
        take = min(left, 2048, x.shape[0])
        out.append(O.make_queries(x, take, seed=seed + i)[0])
        left -= take
        i += 1
    return np.concatenate(out)


@lru_cache(maxsize=3)
def _pool(kind: str, n: int, m: int, k: int = 0) -> dict:
    """kind "ip": unit rows;  "l2": rows of norm 0.8 .. 1.25, raw queries;  "cosine": rows of norm 0.1 .. 3 and queries of norm
    0.5 .. 2 (the index normalises both; the margins are those of the normalised vectors);  "deep" (k given): unit rows with
    DEEP_CLUSTERS clusters of exactly k rows -- the centre and k - 1 rows at noise 0.2 .. 0.6 / sqrt(384) around it -- and
    DEEP_PER_CLUSTER queries per cluster at centre + 0.02 * noise: a random background cannot separate its k-th from its K'-th
    best at k = 100, a query whose top k is one cluster does."""
    rng = np.random.default_rng(zlib.crc32(f"{kind}-{n}-{m}-{k}".encode()))
    x = O.make_corpus(n, seed=1234 + n % 1000)
    reserved = np.zeros(n, bool)              # rows no duplicate cluster may copy
    if kind == "deep":
        assert m <= DEEP_CLUSTERS * DEEP_PER_CLUSTER and 1000 + (DEEP_CLUSTERS - 1) * 3900 + 31 * (k - 1) < n
        qs = []
        for j in range(DEEP_CLUSTERS):
            rows = 1000 + j * 3900 + 31 * np.arange(k)
            centre = x[rows[0]]
            amp = rng.uniform(0.2, 0.6, (k - 1, 1)).astype(np.float32) / np.float32(np.sqrt(384.0))
            x[rows[1:]] = _unit32(centre[None, :] + amp * rng.standard_normal((k - 1, 384), dtype=np.float32))
            reserved[rows] = True
            qs.append(_unit32(centre[None, :] + np.float32(0.02) * rng.standard_normal((DEEP_PER_CLUSTER, 384), dtype=np.float32)))
        q = np.concatenate(qs)[rng.permutation(DEEP_CLUSTERS * DEEP_PER_CLUSTER)[:m]]
        xs, qsearch, metric = x, q, "ip"
    elif kind == "ip":
        q = _planted(x, m, 99)
        xs, qsearch, metric = x, q, "ip"
    elif kind == "l2":
        x = np.ascontiguousarray(x * rng.uniform(0.8, 1.25, (n, 1)).astype(np.float32))
        q = np.ascontiguousarray(x[rng.permutation(n)[:m]] + np.float32(0.05) * rng.standard_normal((m, 384), dtype=np.float32))
        xs, qsearch, metric = x, q, "l2"
    elif kind == "cosine":
        q = _planted(x, m, 99) * rng.uniform(0.5, 2.0, (m, 1)).astype(np.float32)
        x = np.ascontiguousarray(x * rng.uniform(0.1, 3.0, (n, 1)).astype(np.float32))
        xs, qsearch, metric = _unit32(x), _unit32(q), "ip"           # what the index stores and searches with
    else:
        raise ValueError(kind)
    depth = KP_DEEP_MAX if kind == "deep" else KP_AT_STEP2
    top_s, top_r = _top_lists(qsearch, xs, depth, metric)
    dx, xn = corpus_maxima(xs)
    eps = eps_numpy(dx, xn, qsearch, l2=(kind == "l2"))
    return dict(x=x, q=q, xs=xs, qs=qsearch, top_s=top_s, top_r=top_r, eps=eps, dx=dx, xn=xn, reserved=reserved, half=0.5 if kind == "l2" else 1.0)


# ---- the cases ------------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    id: str
    nb: int                       # queries in the request (one block unless it exceeds MAX_QUERIES_PER_LAUNCH)
    c: tuple                      # flagged queries per block
    k: int = 10
    metric: str = "ip"
    n: int = 20_000               # rows of the base corpus (the duplicate clusters are appended to it)
    overflow: bool = False        # one of the flagged queries is the fp16-overflow kind instead of a tie
    row_base: int = 0
    tomb: bool = False            # a third of every cluster's copies is deleted before the search
    copies: int = 0               # appended copies per cluster (0: K' + 8)
    graded: int = 0               # this many flagged queries get a GRADED cluster (see build): a wrong answer unless they are re-run

    @property
    def count(self) -> int:
        return sum(self.c)

    @property
    def kp(self) -> int:
        return screen_kp(self.k)

    @property
    def classes(self) -> list:
        return [rerun_class(nbb, cb)[0] for (_, nbb), cb in zip(blocks(self.nb), self.c)]

    @property
    def kind(self) -> str:
        return "deep" if self.n >= DEEP_N else self.metric

    @property
    def min_batch(self) -> int:
        """set_screen_min_batch(1) where the default heuristics would not screen some block of this request"""
        return 0 if all(path(self.n, nbb, self.k, SCREEN_DIM) == "screen" for _, nbb in blocks(self.nb)) else 1


def _ip(nb, c, **kw):
    """A case of the inner-product table.  A single flagged query has a graded cluster; from two on, one is the overflow kind and
    up to four have graded clusters: a query that is exactly tied keeps a RIGHT answer when no launch re-runs it (the re-score ranks the K' lowest ids
    of its cluster exactly as the exact scan does), so a count that nobody answers would pass unseen; these two kinds do not."""
    n = kw.pop("n", WIDE_ROWS if nb > 1024 else 20_000)      # wide batches over a small corpus: the oracle's cost is nb * n
    tag = kw.pop("tag", "")
    kw.setdefault("overflow", c >= 2)
    kw.setdefault("graded", 1 if c == 1 else min(4, max(0, c - 2)))
    return Case(f"ip-nb{nb}-c{c}-{rerun_class(nb, c)[0]}{tag}", nb, (c,), n=n, **kw)


WIDE_ROWS = 16_384           # (not smaller: 160 cluster bases sit in the K' best rows of a third of the candidates already)
_TABLE = {1: (0, 1), 7: (1, 7), 32: (0, 1, 32), 33: (0, 1, 4, 5, 33), 130: (16, 17), 256: (32, 33), 263: (32, 33), 264: (32, 33, 34),
          300: (1, 37, 38), 1024: (0, 1, 31, 32, 33, 127, 128, 129, 1024), 8192: (1024, 1025)}


def _cross(prefix, **kw):
    """one small-, one mid- and one whole-class count at nb = 1024, and one flagged query at nb = 7"""
    return [Case(f"{prefix}-nb{nb}-c{c}-{rerun_class(nb, c)[0]}", nb, (c,), **kw) for nb, c in ((1024, 5), (1024, 40), (1024, 129), (7, 1))]


DEEP_ROWS = 270_000
CASES = (
    [_ip(nb, c) for nb, cs in _TABLE.items() for c in cs]
    + [_ip(130, 9, overflow=False, graded=0, tag="-ties"), _ip(1024, 40, overflow=False, graded=0, tag="-ties"),
       _ip(264, 33, overflow=False, graded=0, tag="-ties")]                     # exact ties only: every answer in ascending ids
    + _cross("k28", k=28)
    + _cross("rowbase", row_base=1_000_000_007)
    + _cross("tomb", tomb=True)
    + _cross("l2", metric="l2")
    + _cross("cosine", metric="cosine")
    + _cross("deep-k100", k=100, n=DEEP_ROWS)
    + [Case("deep-k100-nb1024-c40-mid-copies136", 1024, (40,), k=100, n=DEEP_ROWS, copies=136)]
    + _cross("deep-k40", k=40, n=DEEP_ROWS)
)

# requests of more than one block: (flagged in block 0, flagged in block 1)
BLOCK_CASES = [
    Case("blocks-8197-mid40-oneclass1", MAX_QUERIES_PER_LAUNCH + 5, (40, 1), n=WIDE_ROWS, overflow=True, graded=4),
    Case("blocks-8492-small3-whole38", MAX_QUERIES_PER_LAUNCH + 300, (3, 38), n=WIDE_ROWS, overflow=True, graded=4),
]
BLOCK_SEAM = tuple(range(8188, 8197))          # rows around the cut that are always compared with the oracle

CPU_MAX_ROWS = 30_000        # the CPU file verifies the verdicts of cases up to this corpus size; the others by the GPU file's control search


# ---- the input builder ----------------------------------------------------------------------------------------------------------
@dataclass
class Built:
    x: np.ndarray                 # the corpus as it is added to the index (clusters appended)
    dead: np.ndarray              # rows to delete before the search
    q: np.ndarray                 # the request
    flagged: np.ndarray           # ascending positions of the flagged queries
    kinds: np.ndarray             # per query: "b" background, "t" tie, "g" graded cluster, "o" fp16 overflow
    margins: np.ndarray           # per query, in EPS: background s_k - s_K'; tie / graded: lead of the cluster over every other row; overflow: inf
    expect: dict                  # position of a tie query -> the k ascending ids of its cluster (without row_base)
    spare: np.ndarray             # a few more certain-pass queries, not in the request
    rep: np.ndarray               # per row of x: itself, or the base row it is a bit-identical copy of (oracle_topk's `rep`)
    graded_rows: dict             # position of a graded query -> ascending ids of its cluster (base row first)

    @property
    def alive(self):
        a = np.ones(self.x.shape[0], bool)
        a[self.dead] = False
        return a


def _positions(rng, nbb: int, cb: int) -> np.ndarray:
    """cb positions in a block of nbb: the last, the first and one adjacent pair first, the rest from a seeded permutation"""
    p = int(rng.integers(1, nbb - 2)) if nbb >= 5 else 0
    forced = []
    for v in (nbb - 1, 0, p, p + 1):
        if 0 <= v < nbb and v not in forced:
            forced.append(v)
    taken = set(forced)
    rest = [int(v) for v in rng.permutation(nbb) if v not in taken]
    return np.sort(np.array((forced + rest)[:cb], np.int64))


N_SPARE = 8


def build(case: Case) -> Built:
    rng = np.random.default_rng(zlib.crc32(case.id.encode()))
    k, kp, count = case.k, case.kp, case.count
    want_bg = case.nb - count + N_SPARE
    m = DEEP_CLUSTERS * DEEP_PER_CLUSTER if case.kind == "deep" else ((3072 if case.metric == "ip" else 2048) if case.nb <= 1024 else 14_336)
    pool = _pool(case.kind, case.n, m, k if case.kind == "deep" else 0)
    x0, n, half = pool["x"], case.n, pool["half"]

    # -- flagged positions, block by block
    flagged = np.concatenate([q0 + _positions(rng, nbb, cb) for (q0, nbb), cb in zip(blocks(case.nb), case.c)]).astype(np.int64)
    overflow_at = int(flagged[count // 2]) if case.overflow else -1
    rest = np.array([p for p in flagged if p != overflow_at], np.int64)
    assert case.graded <= rest.size and (case.graded == 0 or (case.metric == "ip" and not case.tomb))
    graded_at = np.sort(rng.permutation(rest)[:case.graded])
    tie_at = np.setdiff1d(rest, graded_at)
    n_tie = tie_at.size

    # -- duplicate clusters: `copies` copies of a base row each, appended cluster after cluster
    n_cl = min(n_tie, MAX_CLUSTERS)
    copies = case.copies or kp + 8
    if case.tomb:
        copies = copies * 3 // 2
    all_bases = rng.choice(np.nonzero(~pool["reserved"])[0], n_cl + case.graded, replace=False)
    bases, gbases = all_bases[:n_cl], all_bases[n_cl:]
    # -- graded clusters (appended behind the tie clusters): copy j of base b is image(b) * (1 + (j + 1) * GRADE_STEP), a row with the
    # SAME fp16 image as b -- every approximate score of the cluster is one number, the query is certain-fail like a tie -- whose
    # exact score against the query image(b) GROWS with the row id, in steps the fp32 chain and the tie rule (1e-6) resolve.  The
    # screen keeps the lowest ids among equal scores, the true top k are the highest: without a re-run the answer is wrong.
    gx, gq = [], []
    for b in gbases:
        img = _image(x0[b:b + 1]).astype(np.float32) / np.float32(64.0)
        rows = (img * (np.float32(1.0) + np.float32(GRADE_STEP) * np.arange(1, copies + 1, dtype=np.float32)[:, None])).astype(np.float32)
        rows = np.where(_image(rows) == _image(img), rows, img)          # (a component that would leave its fp16 cell stays put)
        assert (_image(rows) == _image(x0[b:b + 1])).all() and (np.diff(rows.astype(np.float64) @ img[0].astype(np.float64)) > 2e-6).all()
        gx.append(rows)
        gq.append(img[0])
    x = np.concatenate([x0] + [np.repeat(x0[b:b + 1], copies, axis=0) for b in bases] + gx) if n_cl + case.graded else x0
    first = n + copies * np.arange(n_cl)
    gfirst = n + copies * (n_cl + np.arange(case.graded))
    rep = np.concatenate([np.arange(n), np.repeat(bases, copies), gfirst[:, None].repeat(copies, 1).ravel() + np.tile(np.arange(copies), case.graded)]).astype(np.int64)
    dx_all, xn_all = pool["dx"], pool["xn"]
    if case.graded:                      # the graded rows may carry the largest image error / norm of the corpus: EPS of the FINAL corpus
        gdx, gxn = corpus_maxima(np.concatenate(gx))
        dx_all, xn_all = max(dx_all, gdx), max(xn_all, gxn)
    eps_bg = eps_numpy(dx_all, xn_all, pool["qs"], l2=(case.metric == "l2")) if case.graded else pool["eps"]
    dead = np.concatenate([f + np.arange(1, copies, 3) for f in first]).astype(np.int64) if case.tomb and n_cl else np.zeros(0, np.int64)
    assert copies - (len(dead) // max(n_cl, 1)) >= kp, "fewer than K' live copies"

    # -- background: candidates whose K' best rows hold no cluster base (a copy then scores at most their K'-th best: the top K'
    # values over the final corpus are those over the base corpus) and whose margin s_k - s_K' is at least 5 EPS
    margin_bg = half * (pool["top_s"][:, k - 1] - pool["top_s"][:, kp - 1]) / eps_bg
    good = (margin_bg >= MARGIN_EPS) & ~np.isin(pool["top_r"][:, :kp], all_bases).any(axis=1)
    if case.graded:                      # a graded row is not a copy: its own score must stay below the candidate's K'-th best
        good &= (pool["qs"].astype(np.float64) @ np.concatenate(gx).astype(np.float64).T).max(axis=1) < pool["top_s"][:, kp - 1]
    pick = np.nonzero(good)[0]
    if pick.size < want_bg + (1 if case.overflow else 0):
        raise RuntimeError(f"{case.id}: {pick.size} certain-pass candidates, {want_bg + 1} needed")
    pick = pick[rng.permutation(pick.size)]
    bg, spare = pick[:case.nb - count], pick[case.nb - count:want_bg]

    q = np.empty((case.nb, 384), np.float32)
    kinds = np.full(case.nb, "b", dtype="<U1")
    margins = np.empty(case.nb)
    is_bg = np.ones(case.nb, bool)
    is_bg[flagged] = False
    q[is_bg] = pool["q"][bg]
    margins[is_bg] = margin_bg[bg]

    # -- tie queries: the base row itself; past MAX_CLUSTERS the clusters are shared and the query is perturbed so that the scores differ
    expect = {}
    if n_tie:
        which = np.arange(n_tie) % n_cl
        tq = x0[bases[which]].copy()
        if n_tie > n_cl:
            assert case.metric == "ip"
            tq = _unit32(tq + np.float32(0.02) * rng.standard_normal(tq.shape, dtype=np.float32))
        q[tie_at] = tq
        kinds[tie_at] = "t"
        # the cluster leads: best row over the base corpus is the base, by >= 5 EPS over the runner-up (which bounds every other cluster too)
        tqs = _unit32(tq) if case.metric == "cosine" else tq
        ts, tr = _top_lists(tqs, pool["xs"], 2, "l2" if case.metric == "l2" else "ip")
        assert (tr[:, 0] == bases[which]).all()
        margins[tie_at] = half * (ts[:, 0] - ts[:, 1]) / eps_numpy(dx_all, xn_all, tqs, l2=(case.metric == "l2"))
        for p, w in zip(tie_at, which):
            live = np.setdiff1d(first[w] + np.arange(copies), dead)
            expect[int(p)] = np.concatenate([[bases[w]], live])[:k].astype(np.int64)
    graded_rows = {}
    if case.graded:
        gqa = np.stack(gq)
        q[graded_at] = gqa
        kinds[graded_at] = "g"
        ts, tr = _top_lists(gqa, pool["xs"], 2, "ip")
        assert (tr[:, 0] == gbases).all()
        # lead of the cluster's LOWEST score (the base row or the first copy) over the best row outside it
        low = np.minimum(ts[:, 0], np.array([float(g[0].astype(np.float64) @ v.astype(np.float64)) for g, v in zip(gx, gq)]))
        margins[graded_at] = (low - ts[:, 1]) / eps_numpy(dx_all, xn_all, gqa)
        for p, b, f in zip(graded_at, gbases, gfirst):
            graded_rows[int(p)] = np.concatenate([[b], f + np.arange(copies)]).astype(np.int64)
    if case.overflow:
        oq = pool["q"][pick[want_bg]] * np.float32(50_000.0)
        assert np.abs(oq).max() * 64.0 > 65504.0                      # fp16(64 q) = inf: eps is not finite
        q[overflow_at] = oq
        kinds[overflow_at] = "o"
        margins[overflow_at] = np.inf
    return Built(x=x, dead=dead, q=q, flagged=np.sort(flagged), kinds=kinds, margins=margins, expect=expect, spare=pool["q"][spare], rep=rep,
                 graded_rows=graded_rows)
