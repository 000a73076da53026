"""CPU: band seeding of the screening ladder (csrc/scan_screen.hip header "Band seeding"), on a numpy emulation of the ladder.

A seeded launch keeps the rows with s~ > threshold (strict).  Today's threshold is the merged K'-th best approximate score; with the band
it is max(K'-th, s~[k-1] - 2 EPS (1 + 2^-10)), each one key step down as the merge and the kernel take them.  The emulation holds a level's
threshold fixed over the level (the kernel's own compactions only raise it towards the same K'-th), counts the rows a level appends, and
checks what the library relies on:
  * every query that passes the sufficiency test has its fp32 top-k (ties by the lower row) inside its candidates, band or not;
  * the flagged set is the same with and without the band;
  * on random rows the seeded levels append at most half as much with the band (K' (ratio - 1) = 224 per level without; the band's edge
    sits near rank 11-12 of 32, which predicts about a third).
EPS is tests/test_screen_bound_cpu.py's."""
import numpy as np
import pytest

from tests.test_screen_bound_cpu import eps, exact_scores_fp32, screen_scores

K, KP = 10, 32
BOUNDS = (256, 2080, 16640, 60000)
N, NQ = BOUNDS[-1], 32
GUARD = np.float32(1.0 + 2.0 ** -10)


def _below(v):
    return np.nextafter(np.float32(v), np.float32(-np.inf))


def _corpus(planted: bool):
    rng = np.random.default_rng(77)
    x = rng.standard_normal((N, 384)).astype(np.float32)
    x /= np.linalg.norm(x, axis=1, keepdims=True)
    q = x[rng.permutation(N)[:NQ]] + 0.1 * rng.standard_normal((NQ, 384)).astype(np.float32)
    if planted:                      # 12..45 near-duplicates of the query direction for 12 queries: 32 or more of them crowd the band
        counts = np.linspace(12, 45, 12).astype(int)
        spots = rng.permutation(N)[:int(counts.sum())]
        at = 0
        for i, c in enumerate(counts):
            d = q[i] / np.linalg.norm(q[i])
            rows = d[None, :] + 2e-3 * rng.standard_normal((c, 384)).astype(np.float32)
            x[spots[at:at + c]] = rows / np.linalg.norm(rows, axis=1, keepdims=True)
            at += c
    return x, q


def _ladder(st_q, e32, band: bool):
    """One query: -> (candidate rows after the last merge (sorted by (-s~, row)), appends per seeded level)."""
    kept = np.zeros(0, np.int64)
    thr = np.float32(-np.inf)
    appends = []
    lo = 0
    for lvl, hi in enumerate(BOUNDS):
        rows = np.arange(lo, hi)
        new = rows[st_q[rows] > thr]
        if lvl > 0:
            appends.append(len(new))
        both = np.concatenate([kept, new])
        kept = both[np.lexsort((both, -st_q[both]))][:KP]
        if len(kept) == KP:                                  # the merged K'-th key exists
            thr = max(thr, _below(st_q[kept[KP - 1]]))       # (u32)(key >> 32), and the kernel's `go - 1u`
            if band and np.isfinite(e32):
                edge = np.float32(st_q[kept[K - 1]] - np.float32(2.0) * e32 * GUARD)
                thr = max(thr, _below(_below(edge)))         # one key step down in the merge, one more in the kernel
        lo = hi
    return kept, appends


def _run(x, q, st, e32, band):
    cand, flagged, appends = [], set(), 0
    for i in range(q.shape[0]):
        kept, app = _ladder(st[i], e32[i], band)
        appends += sum(app)
        s = st[i, kept]
        ok = np.isfinite(e32[i]) and (len(kept) < KP or s[KP - 1] < s[K - 1] - np.float32(2.0) * e32[i])
        if not ok:
            flagged.add(i)
        cand.append(kept)
    return cand, flagged, appends


def _exact_topk(x, q_i, k):
    """fp32 top-k in the exact kernel's k-ordered chain, ties by the lower row.  The chain is within 384 * 2^-24 |x||q| = 2.3e-5 |q| of the fp64
    score, so only rows within 4e-4 of the fp64 k-th best can be in it: the chain runs on those."""
    s64 = x.astype(np.float64) @ q_i.astype(np.float64)
    near = np.nonzero(s64 >= np.sort(s64)[-k] - 4e-4)[0]
    s32 = exact_scores_fp32(x[near], q_i[None, :])[0]
    return set(near[np.lexsort((near, -s32))][:k].tolist())


@pytest.fixture(scope="module", params=[False, True], ids=["random", "planted near-duplicates"])
def world(request):
    x, q = _corpus(request.param)
    st = screen_scores(x, q)
    e32 = eps(x, q).astype(np.float32)
    return request.param, x, q, st, _run(x, q, st, e32, False), _run(x, q, st, e32, True)


def test_passing_queries_hold_their_exact_topk(world):
    planted, x, q, st, off, on = world
    for cand, flagged, _ in (off, on):
        for i in range(NQ):
            if i not in flagged:
                assert _exact_topk(x, q[i], K) <= set(cand[i].tolist()), i
    assert len(on[1]) < NQ


def test_flagged_set_is_the_same(world):
    planted, x, q, st, off, on = world
    assert off[1] == on[1]
    if planted:
        assert 1 <= len(on[1]) <= 12 and on[1] <= set(range(12))        # the crowded bands, and only they
    else:
        assert not on[1]


def test_band_halves_the_appends_on_random_rows(world):
    planted, x, q, st, off, on = world
    print(f"appends over the seeded levels: {off[2]} without the band, {on[2]} with ({on[2] / off[2]:.3f})")
    assert on[2] <= off[2]
    if not planted:
        assert on[2] <= 0.5 * off[2]
