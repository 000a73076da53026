"""CPU: why a spill launch's waves may stop re-reading their thresholds (csrc/scan_screen.hip "Refresh", RMU_OPT_SCREEN_REFRESH), restated in
numpy on the ladder of tests/test_screen_spill_cpu.py (60 000 rows x 32 queries = one wave of an 8-wave workgroup, k = 10, K' = 32).

Inside a seeded launch a query's shared word rises only when some wave that fell back compacts a slot: to one key step below the K'-th
best of rows of this range it has seen, never above.  Two waves filter every level here:
  * the STALE wave keeps the word the launch started with for the whole launch (what option 0 leaves a spilling wave with);
  * the LIVE wave sees the word raised at arbitrary tiles, each time to the K'-th best of the range's rows up to some tile.
Checked per level: the stale wave spills a superset of the live wave's records; the sift, which tests every score strictly against the word
as it stands AFTER the launch, leaves both with the same merged keys, and those keys and the seeds of the next launch are the ones append +
merge produce."""
import numpy as np
import pytest

from tests.test_screen_band_cpu import BOUNDS, KP, NQ, _below, _corpus
from tests.test_screen_bound_cpu import eps, screen_scores
from tests.test_screen_spill_cpu import Q_OF, ROW_OF, _append_and_merge, _flagged, _merge, _plan, _seed, _sift


def _launch(st, lo, hi, thr_tiles):
    """One seeded launch of the wave with room for every record; thr_tiles[t, i] = query i's threshold while tile t is filtered.
    -> (tiles per chunk, records per chunk)"""
    tiles = -(-(hi - lo) // 32)
    s, tpc = _plan(tiles)
    acc = np.zeros((NQ, tiles * 32), np.float32)            # rows past the corpus: the image's slack (zeros)
    m = min(st.shape[1], lo + tiles * 32) - lo
    acc[:, :m] = st[:, lo:lo + m]
    acc = acc.reshape(NQ, tiles, 32).transpose(1, 2, 0)     # [tile, row, query]
    nat = acc[:, ROW_OF[:, None, :], Q_OF[:, :, None]]      # [tile, lane, group, element]: what a lane holds
    passes = nat.max(-1) > thr_tiles[:, Q_OF]               # a lane's running maximum against its group's threshold of that moment
    lists = []
    for c in range(s):
        recs = []
        for t in range(c * tpc, min((c + 1) * tpc, tiles)):
            for g in range(2):
                for lane in np.nonzero(passes[t, :, g])[0]:
                    recs.append((t - c * tpc, int(lane), g, nat[t, lane, g].copy()))
        lists.append(recs)
    return tpc, lists


def _raised(rng, st, lo, hi, thr):
    """-> (thr_tiles [tiles, NQ], raises): per query the launch's word, raised at up to three arbitrary tiles to one key step below the K'-th
    best of the rows [lo, end of that tile) above the launch's word -- a compaction's publication; no raise where fewer than K' exist."""
    tiles = -(-(hi - lo) // 32)
    thr_tiles = np.repeat(thr[None, :], tiles, axis=0).astype(np.float32)
    raises = 0
    for i in range(NQ):
        for t in sorted(rng.choice(tiles, size=min(3, tiles), replace=False)):
            rows = np.arange(lo, min(hi, lo + 32 * (t + 1)))
            s = st[i, rows]
            s = np.sort(s[s > thr[i]])[::-1]
            if len(s) >= KP and _below(s[KP - 1]) > thr_tiles[t, i]:
                thr_tiles[t + 1:, i] = _below(s[KP - 1])    # seen from the next tile on
                raises += t + 1 < tiles
    return thr_tiles, raises


@pytest.fixture(scope="module", params=[False, True], ids=["random", "planted near-duplicates"])
def world(request):
    x, q = _corpus(request.param)
    return request.param, screen_scores(x, q), eps(x, q).astype(np.float32)


@pytest.mark.parametrize("last", [BOUNDS[-1], BOUNDS[-1] - 10], ids=["whole tiles", "partial last tile"])
def test_a_stale_wave_spills_a_superset_and_the_sift_leaves_the_same_keys_and_seeds(world, last):
    planted, st, e32 = world
    bounds = BOUNDS[:-1] + (last,)
    ref = _append_and_merge(st, e32, bounds)
    rng = np.random.default_rng(5)
    kept = {w: [np.zeros(0, np.int64) for _ in range(NQ)] for w in ("stale", "live")}
    thr = np.full(NQ, -np.inf, np.float32)
    lo, raises, dropped = 0, 0, 0
    for lvl, hi in enumerate(bounds):
        if lvl == 0:                                        # the cold first launch stays as it is
            rows = np.arange(lo, hi)
            for w in kept:
                for i in range(NQ):
                    kept[w][i] = _merge(st[i], kept[w][i], rows[st[i, rows] > thr[i]])
            final = thr
        else:
            thr_tiles, n_raised = _raised(rng, st, lo, hi, thr)
            raises += n_raised
            assert (np.diff(thr_tiles, axis=0) >= 0).all() and (thr_tiles[0] == thr).all()      # thresholds only rise
            final = thr_tiles[-1]                           # the word after the launch
            tpc, stale = _launch(st, lo, hi, np.repeat(thr[None, :], len(thr_tiles), axis=0))
            tpc2, live = _launch(st, lo, hi, thr_tiles)
            assert tpc == tpc2 and len(stale) == len(live)
            for a, b in zip(stale, live):                   # per chunk: the live wave's records are among the stale wave's
                ka, kb = {r[:3] for r in a}, {r[:3] for r in b}
                assert kb <= ka
                dropped += len(ka - kb)
            parts = [None] * len(stale)
            for i in range(NQ):
                kept["stale"][i] = _sift(i, st[i], kept["stale"][i], final[i], lo, hi, tpc, stale, parts)
                kept["live"][i] = _sift(i, st[i], kept["live"][i], final[i], lo, hi, tpc, live, parts)
        thr = np.array([_seed(final[i], kept["stale"][i], st[i], e32[i]) for i in range(NQ)], np.float32)
        thr_live = np.array([_seed(final[i], kept["live"][i], st[i], e32[i]) for i in range(NQ)], np.float32)
        for i in range(NQ):
            assert np.array_equal(kept["stale"][i], kept["live"][i]), (lvl, i)
            assert np.array_equal(kept["stale"][i], ref[lvl][0][i]), (lvl, i)
        assert np.array_equal(thr, thr_live) and np.array_equal(thr, ref[lvl][1]), lvl
        lo = hi
    assert _flagged(st, e32, kept["stale"]) == _flagged(st, e32, ref[-1][0])
    print(f"{raises} raises, {dropped} records only the stale wave wrote")
    assert raises > 0 and dropped > 0                       # the words did rise, and the live wave did filter more
