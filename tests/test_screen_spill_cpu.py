"""CPU: the spill path of the screening ladder (csrc/scan_screen.hip "Spill path", csrc/topk_merge.hip sift_kernel), restated
in numpy on the ladder of tests/test_screen_band_cpu.py (60 000 rows x 32 queries = one wave of an 8-wave workgroup, k = 10, K' = 32).

A seeded launch used to append every score above the query's threshold inside the tile loop (slow_path) and a merge folded the per-chunk
lists into the running top-K'.  With the spill path a LANE whose maximum over the 8 scores it holds of a query group beats the group's
threshold writes those 8 scores, as the 16x16x32 MFMA left them, with (tile of the chunk, lane, group) into the wave's list of the chunk;
the sift kernel afterwards picks a query's records, turns (chunk, tile, lane, group, element) into the row, drops what is not strictly
above the threshold or lies past the range, and merges with the running top-K'.  A list that cannot take a tile's records ends the wave's
spilling: that tile and the rest of the chunk go through slow_path and reach the sift as a part list.  Checked here:
  * per level the same merged keys and the same thresholds as append + merge, and the same flagged queries at the end -- with room for
    every record, with 128 and with 4 records per list (waves fall back in the middle of a launch), and with a last range that ends in a partial tile;
  * every candidate the sift builds carries the score of the row it names;
  * record -> (row, query) for all 64 lanes x 2 groups x 8 elements against the ownership tables of tests/test_screen_shape_cpu.py: the MFMA's
    own layout, and slow_path's rows behind the eight half-swaps."""
import numpy as np
import pytest

from tests.test_screen_band_cpu import BOUNDS, GUARD, K, KP, NQ, _below, _corpus
from tests.test_screen_bound_cpu import eps, screen_scores
from tests.test_screen_shape_cpu import native_layout, to_owner

LANES = np.arange(64)
ELEMS = np.arange(8)
ROW_OF = 16 * (ELEMS[None, :] >> 2) + 4 * (LANES[:, None] >> 4) + (ELEMS[None, :] & 3)     # [lane, element] -> row of the tile
Q_OF = 16 * np.arange(2)[None, :] + (LANES[:, None] & 15)                                  # [lane, group] -> query of the wave
CHUNKS = 8


# ---- record -> (row, query) ---------------------------------------------------------------------------------------------------------------
def test_record_arithmetic_is_the_mfma_layout_and_slow_paths_rows():
    nat = native_layout()                                   # [8 g + 4 t + c, lane] -> (query, row)
    for lane in range(64):
        for g in range(2):
            for e in range(8):
                assert tuple(nat[8 * g + e, lane]) == (Q_OF[lane, g], ROW_OF[lane, e]), (lane, g, e)
    # slow_path, behind to_owner: the lane of query j holds row 4 h + 8 i + c at element 4 i + c and stores key row rbase + (r & 3) + 8 (r >> 2)
    # with rbase = ... + 4 h: the same 1024 (query, row) cells, each once
    own = to_owner(nat)
    cells = set()
    for lane in range(64):
        h, j = (lane >> 4) & 1, 16 * (lane >> 5) + (lane & 15)
        for r in range(16):
            assert tuple(own[r, lane]) == (j, 4 * h + (r & 3) + 8 * (r >> 2))
            cells.add((j, 4 * h + (r & 3) + 8 * (r >> 2)))
    assert cells == {(int(Q_OF[lane, g]), int(ROW_OF[lane, e])) for lane in range(64) for g in range(2) for e in range(8)}
    assert len(cells) == 1024


# ---- the ladder, both ways ----------------------------------------------------------------------------------------------------------------
def _seed(thr, kept, st_q, e32):
    """the merge's / the sift's seeding of the next launch (tests/test_screen_band_cpu.py: _ladder)"""
    if len(kept) == KP:
        thr = max(thr, _below(st_q[kept[KP - 1]]))
        if np.isfinite(e32):
            thr = max(thr, _below(_below(np.float32(st_q[kept[K - 1]] - np.float32(2.0) * e32 * GUARD))))
    return thr


def _merge(st_q, kept, new):
    both = np.concatenate([kept, np.asarray(new, np.int64)])
    return both[np.lexsort((both, -st_q[both]))][:KP]


def _append_and_merge(st, e32, bounds):
    """-> per level (merged rows per query, thresholds per query)"""
    kept = [np.zeros(0, np.int64) for _ in range(NQ)]
    thr = np.full(NQ, -np.inf, np.float32)
    out, lo = [], 0
    for hi in bounds:
        rows = np.arange(lo, hi)
        for i in range(NQ):
            kept[i] = _merge(st[i], kept[i], rows[st[i, rows] > thr[i]])
            thr[i] = _seed(thr[i], kept[i], st[i], e32[i])
        out.append(([k.copy() for k in kept], thr.copy()))
        lo = hi
    return out


def _plan(tiles):
    s = min(CHUNKS, tiles)
    tpc = -(-tiles // s)
    return -(-tiles // tpc), tpc


def _spill_launch(st, lo, hi, thr, cap):
    """One seeded launch of the wave: -> (chunks, tiles per chunk, records per chunk, part lists of the chunks whose list ran full)."""
    tiles = -(-(hi - lo) // 32)
    s, tpc = _plan(tiles)
    acc = np.zeros((NQ, tiles * 32), np.float32)            # rows past the corpus: the image's slack (zeros)
    m = min(st.shape[1], lo + tiles * 32) - lo
    acc[:, :m] = st[:, lo:lo + m]
    acc = acc.reshape(NQ, tiles, 32).transpose(1, 2, 0)     # [tile, row, query]
    nat = acc[:, ROW_OF[:, None, :], Q_OF[:, :, None]]      # [tile, lane, group, element]: what a lane holds
    passes = nat.max(-1) > thr[Q_OF][None]                  # a lane's running maximum against its group's threshold
    lists, parts = [], []
    for c in range(s):
        recs, part = [], None
        t_end = min((c + 1) * tpc, tiles)
        for t in range(c * tpc, t_end):
            p = passes[t]
            if not p.any():
                continue
            if len(recs) + int(p.sum()) > cap:              # the tile does not fit: slow_path for it and the rest of the chunk
                r0, r1 = lo + t * 32, min(hi, lo + t_end * 32)
                rows = np.arange(r0, r1)
                part = [_merge(st[i], np.zeros(0, np.int64), rows[st[i, rows] > thr[i]]) for i in range(NQ)]
                break
            for g in range(2):
                for lane in np.nonzero(p[:, g])[0]:
                    recs.append((t - c * tpc, int(lane), g, nat[t, lane, g].copy()))
        lists.append(recs)
        parts.append(part)
    return s, tpc, lists, parts


def _sift(i, st_q, kept, thr_q, lo, hi, tpc, lists, parts):
    new = []
    for c, recs in enumerate(lists):
        for tile, lane, g, v in recs:
            if (lane & 15) != (i & 15) or g != (i >> 4):
                continue
            for e in range(8):
                row = lo + (c * tpc + tile) * 32 + 16 * (e >> 2) + 4 * (lane >> 4) + (e & 3)
                if v[e] > thr_q and row < hi:
                    assert v[e] == st_q[row], (i, c, tile, lane, g, e)          # the score belongs to the row the arithmetic names
                    new.append(row)
        if parts[c] is not None:
            new += parts[c][i].tolist()
    assert len(new) == len(set(new))
    return _merge(st_q, kept, new)


def _spill_and_sift(st, e32, bounds, cap):
    kept = [np.zeros(0, np.int64) for _ in range(NQ)]
    thr = np.full(NQ, -np.inf, np.float32)
    out, lo, records, fell = [], 0, 0, 0
    for lvl, hi in enumerate(bounds):
        if lvl == 0:                                        # the cold first launch stays as it is
            rows = np.arange(lo, hi)
            for i in range(NQ):
                kept[i] = _merge(st[i], kept[i], rows[st[i, rows] > thr[i]])
        else:
            s, tpc, lists, parts = _spill_launch(st, lo, hi, thr, cap)
            records += sum(len(r) for r in lists)
            fell += sum(p is not None for p in parts)
            for i in range(NQ):
                kept[i] = _sift(i, st[i], kept[i], thr[i], lo, hi, tpc, lists, parts)
        for i in range(NQ):
            thr[i] = _seed(thr[i], kept[i], st[i], e32[i])
        out.append(([k.copy() for k in kept], thr.copy()))
        lo = hi
    return out, records, fell


def _flagged(st, e32, kept):
    bad = set()
    for i in range(NQ):
        s = st[i, kept[i]]
        if not (np.isfinite(e32[i]) and (len(kept[i]) < KP or s[KP - 1] < s[K - 1] - np.float32(2.0) * e32[i])):
            bad.add(i)
    return bad


@pytest.fixture(scope="module", params=[False, True], ids=["random", "planted near-duplicates"])
def world(request):
    x, q = _corpus(request.param)
    st = screen_scores(x, q)
    e32 = eps(x, q).astype(np.float32)
    return request.param, st, e32, {}


def _reference(world, bounds):
    _, st, e32, cache = world
    if bounds not in cache:
        cache[bounds] = _append_and_merge(st, e32, bounds)
    return cache[bounds]


@pytest.mark.parametrize("cap", [1 << 20, 128, 4], ids=["room for every record", "128 records per list", "4 records per list"])
@pytest.mark.parametrize("last", [BOUNDS[-1], BOUNDS[-1] - 10], ids=["whole tiles", "partial last tile"])
def test_spill_and_sift_is_append_and_merge(world, cap, last):
    planted, st, e32, _ = world
    bounds = BOUNDS[:-1] + (last,)
    ref = _reference(world, bounds)
    got, records, fell = _spill_and_sift(st, e32, bounds, cap)
    print(f"{records} records, {fell} lists ran full")
    for lvl, ((rk, rt), (gk, gt)) in enumerate(zip(ref, got)):
        for i in range(NQ):
            assert np.array_equal(rk[i], gk[i]), (lvl, i)
        assert np.array_equal(rt, gt), lvl
    assert _flagged(st, e32, ref[-1][0]) == _flagged(st, e32, got[-1][0])
    if planted:
        assert _flagged(st, e32, got[-1][0])                # the crowded bands are flagged either way
    assert records > 0
    assert (fell > 0) == (cap <= 128)                       # 128: lists that fill up in the middle of a chunk; 4: at the first passing tile
    if cap == 128:
        assert records > 20 * 128
