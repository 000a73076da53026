"""GPU: the tile loop of the 8-wave screening kernels (csrc/scan_screen.hip) -- whole ring periods of six unconditional tile bodies, one
conditional remainder period, and the workgroup paced by one of its early waves -- changes no answer.

Every case is the screened search against the exact fp32 scan (k = 112 is beyond the screening path: the exact scan answers it, and its
first k columns are the exact top-k, ties by row id): same ids, same score bits.  Option 10 = 1 (every wave reads its thresholds at every pair:
the pacing wave's prologue on all eight) must return the same bits and re-run the same number of queries as the default.

Shapes.  set_ladder(8, 256) gives the ranges n/64, n/8, n (multiples of 32, each at least 256 rows); the LAST range, n - (n/8 rounded down to 32),
is the launch whose geometry last_geometry() reports, and the planner (rmu_common.h: rmu_plan_chunks, scan_screen.hip: rmu_screen_plan) is
restated below to turn the reported grid into tiles per chunk.  With 1024 queries (four query tiles, 64 row chunks) the six small corpora
give 5, 6, 7, 8, 9 and 10 tiles per chunk: fewer than a period, exactly one, one and a remainder of one, and with 32 every class of
tiles_per_chunk % 6; with 257 and 300 queries (two query tiles, up to 128 chunks) the same corpora run 3 to 5 tiles per chunk -- the
remainder period alone.  74 864 rows is the smallest corpus whose last range paces at four query tiles (64 chunks x 32 tiles of 32 rows;
the last tile is half empty), 149 780 rows the smallest at two (128 x 32), where 1024 queries run 64 tiles per chunk."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu

SMALL = (11_003, 13_001, 15_003, 17_501, 19_507, 22_001)      # 1024 queries: 5, 6, 7, 8, 9, 10 tiles per chunk of the last range
PACED4, PACED2 = 74_864, 149_780
BATCHES = (257, 300, 1024)
KS = (10, 40)                                                  # K' = 32 and the DEEP slots
PACE_WINDOW = 8                                                # RMU_SCREEN_PACE's default
SEED = 131


def last_range(n):
    """set_ladder(8, 256) below 512k rows (rmu_api.hip: ladder_bounds): rows of the last launch."""
    assert 4096 <= n < 8 * 65536
    return n - n // 8 // 32 * 32


def plan(nq, rows, n_cu):
    """rmu_plan_chunks + rmu_screen_plan for an 8-wave launch: (query tiles, row chunks, tiles per chunk, paced)."""
    nqt, tiles = (nq + 255) // 256, (rows + 31) // 32
    best_s, best = 8, -1.0
    for s in range(8, 257, 8):
        tot = s * nqt
        eff = tot / (((tot + 255) // 256) * 256)
        if eff > best + 1e-9:
            best, best_s = eff, s
        if tot >= 256 and eff > 0.999:
            break
    s = min(best_s, max(tiles, 1))
    tpc = max(1, (tiles + s - 1) // s)
    used = (tiles + tpc - 1) // tpc
    if 0 < used < s:
        s = used
    paced = 2 <= nqt <= 4 and s % 8 == 0 and s * nqt <= n_cu and tpc >= 4 * PACE_WINDOW
    return nqt, s, tpc, paced


@pytest.fixture(scope="module")
def rmu():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import ragmeup_amd
    from ragmeup_amd import _native
    _native.lib()
    return ragmeup_amd


def _index(rmu, x, metric="ip"):
    from ragmeup_amd import _native as N
    idx = rmu.FlatIndex(384, metric={"ip": N.METRIC_IP, "cosine": N.METRIC_COSINE, "l2": N.METRIC_L2SQ}[metric])
    idx.set_ladder(8, 256)
    idx.add(x)
    return idx


@pytest.fixture(scope="module")
def world(rmu):
    """Corpora, queries, indexes and the exact scan's answers, made once and shared (no test modifies them)."""
    import torch
    corpora, indexes, exact = {}, {}, {}

    def get(n, metric, nq):
        if n not in corpora:
            x = O.make_corpus(n, seed=SEED)
            corpora[n] = (x, torch.from_numpy(O.make_queries(x, 1024, seed=SEED + 1)[0]).cuda())
        if (n, metric) not in indexes:
            indexes[(n, metric)] = _index(rmu, corpora[n][0], metric)
        idx, q = indexes[(n, metric)], corpora[n][1][:nq]
        if (n, metric, nq) not in exact:
            se, re_ = idx.search(q, 112)
            assert idx.last_screened() == 0, "k = 112 is the exact scan's"
            exact[(n, metric, nq)] = (se.clone(), re_.clone())
        return idx, q, exact[(n, metric, nq)]

    yield get
    for idx in indexes.values():
        idx.close()


def n_cu():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def check(idx, q, ref, k, n=0):
    """The default and option 10 = 1 against the exact scan: same bits, same re-run count.  -> (tiles per chunk, paced) of the ladder's last
    launch when the corpus size n is given and no query was re-run (the last scan enqueued is then that launch, and its grid must be the
    planner's), else None: a query whose K' candidates all lie inside the band is answered by the exact scan, whose geometry is reported."""
    import torch
    se, re_ = ref
    got, shape = {}, None
    try:
        for refresh in (False, True):
            idx.set_screen_refresh(refresh)
            s, r = idx.search(q, k)
            got[refresh] = idx.last_screened()
            assert got[refresh] != 0, "expected the screening path"
            assert torch.equal(r, re_[:, :k]) and torch.equal(s, se[:, :k]), f"option 10 = {int(refresh)}, k = {k}: not the exact scan's bits"
            if n and not refresh and got[refresh] > 0:
                geo = idx.last_geometry()
                nqt, s_chunks, tpc, paced = plan(q.shape[0], last_range(n), n_cu())
                shape = (tpc, paced)
                assert geo["block"] == 256 and geo["grid"] == s_chunks * nqt, (geo, nqt, s_chunks, tpc)
                assert geo["launches"] >= 2
    finally:
        idx.set_screen_refresh(False)
    assert got[False] == got[True], got
    return shape


def shape_of(shapes):
    """The geometry of a (corpus, batch) from the searches of it that re-ran no query: at least one k must be such a search."""
    seen = {sh for sh in shapes if sh is not None}
    assert len(seen) == 1, shapes
    return seen.pop()


def test_the_planner_restated_here_gives_the_shapes_the_cases_are_named_for():
    """(arithmetic only; the GPU cases below check the grid it predicts against the grid that ran)"""
    tpcs = [plan(1024, last_range(n), 256)[2] for n in SMALL]
    assert tpcs == [5, 6, 7, 8, 9, 10]
    assert {t % 6 for t in tpcs} == set(range(6))
    assert all(plan(nq, last_range(n), 256)[2] < 6 for n in SMALL for nq in (257, 300))
    assert plan(1024, last_range(PACED4), 256) == (4, 64, 32, True) and last_range(PACED4) % 32 == 16
    assert plan(1024, last_range(PACED4) - 32 * 64, 256)[3] is False          # one tile per chunk less: not paced -- the smallest that is
    assert plan(257, last_range(PACED2), 256) == (2, 128, 32, True)
    assert plan(1024, last_range(PACED2), 256) == (4, 64, 64, True)
    assert not any(plan(nq, last_range(PACED4), 256)[3] for nq in (257, 300))


@pytest.mark.parametrize("metric", ("ip", "l2"))
@pytest.mark.parametrize("n", SMALL)
def test_period_and_remainder_split(world, n, metric):
    """Fewer than six tiles per chunk, exactly six, seven, and every remainder 0..5 at four query tiles; the remainder period alone at two.
    (L2 as well: its kernels read each tile's row norms a tile ahead, and the last body of a remainder reads norms nobody uses.)"""
    seen = {}
    for nq in BATCHES:
        idx, q, ref = world(n, metric, nq)
        seen[nq] = shape_of([check(idx, q, ref, k, n) for k in KS])
    tpc = seen[1024][0]
    assert tpc == 5 + SMALL.index(n), seen                     # 5 (< 6), 6, 7, then 8, 9, 10: tiles_per_chunk % 6 = 5, 0, 1, 2, 3, 4
    assert all(seen[nq][0] < 6 for nq in (257, 300)), seen
    assert not any(p for _, p in seen.values())


@pytest.mark.parametrize("metric", ("ip", "cosine", "l2"))
def test_paced_launch_of_four_query_tiles(world, metric):
    """64 chunks x 32 tiles, four sibling workgroups per chunk: rmu_screen_plan's condition holds for the last launch with 1024 queries, and
    not with 257 or 300 (16 to 17 tiles per chunk), which run the same corpus unpaced."""
    for nq in BATCHES:
        idx, q, ref = world(PACED4, metric, nq)
        tpc, paced = shape_of([check(idx, q, ref, k, PACED4) for k in KS])
        if nq == 1024:                                         # (check() has set the planner's grid against the grid that ran)
            nqt, s_chunks, _, _ = plan(nq, last_range(PACED4), n_cu())
            assert 2 <= nqt <= 4 and s_chunks % 8 == 0 and s_chunks * nqt <= n_cu() and tpc >= 4 * PACE_WINDOW and paced
            assert tpc % 6 == 2
        else:
            assert not paced and tpc in (16, 17)


def test_paced_launch_of_two_query_tiles_the_second_almost_empty(world):
    """257 queries: the second sibling holds one query -- its pacing wave has none -- and still publishes and paces (128 chunks x 32 tiles);
    300 queries likewise; 1024 queries run 64 tiles per chunk, ten periods and a remainder of four."""
    for nq, want in ((257, 32), (300, 32), (1024, 64)):
        idx, q, ref = world(PACED2, "ip", nq)
        tpc, paced = shape_of([check(idx, q, ref, k, PACED2) for k in KS])
        assert paced and tpc == want, (nq, tpc, paced)


def _clustered(n, seed):
    """n rows, 1024 queries; 100 rows within 1e-4 .. 1e-3 of queries 3, 150 and 700 (group 0 of wave 0, group 1 of wave 4, the third sibling)
    in 100 CONSECUTIVE rows of the last range: the wave that meets them passes in four tiles running, falls back when its list is short,
    compacts and raises the shared word while its workgroup is being paced."""
    rng = np.random.default_rng(seed)
    x = O.make_corpus(n, seed=seed + 1)
    q = O.make_corpus(1024, seed=seed + 2)
    deficit = np.linspace(1e-4, 1e-3, 100)
    spots = {}
    for i, tile in ((3, 400), (150, 1111), (700, 2100)):
        rows = q[i][None, :] + np.sqrt(2.0 * deficit / 383.0)[:, None].astype(np.float32) * rng.standard_normal((100, 384)).astype(np.float32)
        spots[i] = np.arange(32 * tile + 5, 32 * tile + 105)
        x[spots[i]] = rows / np.linalg.norm(rows, axis=1, keepdims=True)
    return x, q, spots


def test_near_duplicates_and_tombstones_while_the_wave_paces(rmu):
    import torch
    x, q, spots = _clustered(PACED4, SEED + 10)
    assert all(rows[0] >= PACED4 - last_range(PACED4) for rows in spots.values())       # all in the paced range
    idx = _index(rmu, x)
    qd = torch.from_numpy(q).cuda()

    def exact():
        ref = idx.search(qd, 112)
        assert idx.last_screened() == 0
        return ref

    def run(k, cap):
        try:
            idx.set_screen_spill(True, cap)
            check(idx, qd, ref, k)
            assert idx.last_screened() <= -3                     # K' rows inside the band: the three queries are answered by the exact scan
            return idx.search(qd, k)[1].cpu().numpy()
        finally:
            idx.set_screen_spill(True, 0)

    try:
        ref = exact()
        for cap in (0, 4):                                       # the default list, and four records per list: waves fall back mid-launch
            for k in KS:
                r = run(k, cap)
                for i, rows in spots.items():
                    assert np.isin(r[i], rows).all()
        dead = np.concatenate([rows[::3] for rows in spots.values()])
        assert idx.remove_rows(dead) == len(dead)
        ref = exact()
        for cap in (0, 4):
            r = run(10, cap)
            assert not np.isin(r, dead).any()
            for i, rows in spots.items():
                assert np.isin(r[i], rows).all()
    finally:
        idx.close()


def test_tombstones_in_every_chunk_of_a_paced_launch(rmu):
    """Every 97th row deleted (each chunk of the paced range loses about ten) on a corpus with a remainder period: deleted rows are never
    returned and the bits are the exact scan's over the live rows."""
    import torch
    x = O.make_corpus(PACED4, seed=SEED + 20)
    q = torch.from_numpy(O.make_queries(x, 1024, seed=SEED + 21)[0]).cuda()
    idx = _index(rmu, x)
    try:
        dead = np.arange(11, PACED4, 97)
        assert idx.remove_rows(dead) == len(dead)
        ref = idx.search(q, 112)
        assert idx.last_screened() == 0
        for k in KS:
            check(idx, q, ref, k)
            assert not np.isin(idx.search(q, k)[1].cpu().numpy(), dead).any()
    finally:
        idx.close()


def test_pacing_switched_off_in_a_child_process_returns_the_same_bits(world):
    """RMU_SCREEN_PACE is read once per process: a fresh interpreter with RMU_SCREEN_PACE=0 searches the paced corpus
    (tests/screen_pace_driver.py) and must return the bits and the re-run count of this process, where the launch is paced."""
    idx, q, ref = world(PACED4, "ip", 1024)
    mine = {}
    assert shape_of([check(idx, q, ref, k, PACED4) for k in KS])[1]
    for k in KS:
        s, r = idx.search(q, k)
        mine[str(k)] = {"screened": idx.last_screened(),
                        "digest": hashlib.sha1(r.cpu().numpy().tobytes() + s.cpu().numpy().tobytes()).hexdigest()}
    here = os.path.dirname(os.path.abspath(__file__))
    out = subprocess.run([sys.executable, os.path.join(here, "screen_pace_driver.py"), str(PACED4), str(SEED)] + [str(k) for k in KS],
                         env=dict(os.environ, RMU_TUNING="1", RMU_SCREEN_PACE="0"), capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    res = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    assert res == mine, (res, mine)
