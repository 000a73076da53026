"""GPU: RMU_OPT_SCREEN_REFRESH (csrc/scan_screen.hip "Refresh") changes no answer.

In a spill launch of the screening ladder a wave re-reads its queries' shared thresholds only while it can use them (option 10 = 0, the
default): at its first pair of tiles, once its spill list is full and it appends and compacts again, and the wave that paces the
workgroup.  Option 10 = 1 makes every wave re-read and refresh them at every pair of tiles.  Every case is searched three ways -- option 0,
option 1 and the exact fp32 scan (RMU_OPT_SCREEN = 0) -- and all three must return the same ids and the same score bits; the two settings
must also re-run the same number of queries (last_screened()).

Shapes: the smallest that run several seeded 8-wave levels (rmu_api.hip: ladder_bounds; below 64k rows the ratio is 8).  131 100 rows with
the default ladder -> 256 / 2 048 / 16 384 / 131 100, and with the (2, 128) ladder of tests/test_screen_spill_gpu.py its five levels;
70 000 rows with set_ladder(3, 256) -> 1 088 / 8 736 / 70 000.  All end in a partial tile.  Batches 129 / 256 / 300 / 1024: one query in the
second wave, one full workgroup, a part-filled second one, four query tiles (sibling pacing).  k = 10 and 28: K' = 32 and 40; k = 40: the
deep slots, also on 300 000 rows, where a deep k screens whatever the batch."""
import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu

LADDERS = {"131100 default": (131_100, 0, 0), "131100 five levels": (131_100, 2, 128), "70000 ratio 3": (70_000, 3, 256)}
BATCHES = (129, 256, 300, 1024)
KS = (10, 28, 40)
METRICS = ("ip", "cosine", "l2")


@pytest.fixture(scope="module")
def rmu():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import ragmeup_amd
    from ragmeup_amd import _native
    _native.lib()
    return ragmeup_amd


def _index(rmu, x, metric="ip", ratio=0, first=0):
    from ragmeup_amd import _native as N
    idx = rmu.FlatIndex(384, metric={"ip": N.METRIC_IP, "cosine": N.METRIC_COSINE, "l2": N.METRIC_L2SQ}[metric])
    idx.set_ladder(ratio, first)
    idx.add(x)
    return idx


@pytest.fixture(scope="module")
def world(rmu):
    """Corpora, queries and indexes, made once and shared (no test modifies them; every test leaves the switches at their defaults)."""
    import torch
    corpora, indexes = {}, {}

    def get(ladder, m):
        n, ratio, first = LADDERS[ladder]
        if n not in corpora:
            x = O.make_corpus(n, seed=91)
            corpora[n] = (x, torch.from_numpy(O.make_queries(x, 1024, seed=92)[0]).cuda())
        if (ladder, m) not in indexes:
            indexes[(ladder, m)] = _index(rmu, corpora[n][0], m, ratio, first)
        return indexes[(ladder, m)], corpora[n][1]

    yield get
    for idx in indexes.values():
        idx.close()


def three_ways(idx, q, k, cap=0, min_launches=3):
    """-> (scores, rows, last_screened) of the option 10 = 0 search, after checking it against option 10 = 1 and the exact scan."""
    import torch
    out = {}
    try:
        idx.set_screen_spill(True, cap)
        for refresh in (False, True):
            idx.set_screen_refresh(refresh)
            s, r = idx.search(q, k)
            out[refresh] = (s, r, idx.last_screened())
            assert out[refresh][2] != 0, f"refresh {refresh}: expected the screening path"
            assert idx.last_geometry()["launches"] >= min_launches
    finally:
        idx.set_screen_refresh(False)
        idx.set_screen_spill(True, 0)
    idx.set_screening(False)
    try:
        se, re_ = idx.search(q, k)
        assert idx.last_screened() == 0
    finally:
        idx.set_screening(True)
    for refresh in (False, True):
        s, r, _ = out[refresh]
        assert torch.equal(r, re_) and torch.equal(s, se), f"refresh {refresh} differs from the exact scan at k = {k}, cap = {cap}"
    assert out[False][2] == out[True][2], (out[False][2], out[True][2])
    return out[False]


def test_the_switch_is_option_ten(rmu):
    from ragmeup_amd import _native as N
    assert N.OPT_SCREEN_REFRESH == 10
    idx = rmu.FlatIndex(384)
    try:
        idx.set_screen_refresh(True)
        idx.set_screen_refresh(False)
    finally:
        idx.close()


@pytest.mark.parametrize("nq", BATCHES, ids=[f"{b}q" for b in BATCHES])
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("ladder", ["131100 default", "70000 ratio 3"])
def test_refresh_on_off_and_exact_scan_agree(world, ladder, metric, nq):
    idx, q = world(ladder, metric)
    for k in KS:
        three_ways(idx, q[:nq], k)


@pytest.mark.parametrize("nq", BATCHES, ids=[f"{b}q" for b in BATCHES])
def test_five_levels(world, nq):
    idx, q = world("131100 five levels", "ip")
    for k in KS:
        three_ways(idx, q[:nq], k, min_launches=5)


@pytest.mark.parametrize("metric", ("ip", "l2"))
def test_deep_slots_on_300k_rows(rmu, metric):
    """k = 40 (K' = 48: the DEEP instantiations) over 300 000 rows with the default ladder, a part-filled second workgroup and four query tiles."""
    import torch
    x = O.make_corpus(300_000, seed=93)
    q = torch.from_numpy(O.make_queries(x, 1024, seed=94)[0]).cuda()
    idx = _index(rmu, x, metric)
    try:
        for nq in (300, 1024):
            for cap in (0, 4):
                three_ways(idx, q[:nq], 40, cap=cap)
    finally:
        idx.close()


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("ladder", ["131100 default", "70000 ratio 3"])
def test_four_records_per_list_fall_back_mid_launch(world, ladder, metric):
    """RMU_OPT_SCREEN_SPILL_CAP = 4: a wave's list takes its first few records, then the wave appends, compacts and reads its thresholds
    again -- first the words of its first refresh, then what its next one brings."""
    idx, q = world(ladder, metric)
    for nq in (300, 1024):
        for k in KS:
            three_ways(idx, q[:nq], k, cap=4)


def _clustered(seed):
    """70 000 rows, 300 queries; 100 rows within 1e-4 .. 1e-3 of queries 3, 150 and 290 (group 0 of wave 0, group 1 of wave 4, the part-filled
    second workgroup) in 100 CONSECUTIVE rows of the last range: the wave that meets them passes in four tiles running."""
    rng = np.random.default_rng(seed)
    x = O.make_corpus(70_000, seed=seed + 1)
    q = O.make_corpus(300, seed=seed + 2)
    deficit = np.linspace(1e-4, 1e-3, 100)
    spots = {}
    for i, tile in ((3, 400), (150, 1111), (290, 2100)):
        rows = q[i][None, :] + np.sqrt(2.0 * deficit / 383.0)[:, None].astype(np.float32) * rng.standard_normal((100, 384)).astype(np.float32)
        spots[i] = np.arange(32 * tile + 5, 32 * tile + 105)
        x[spots[i]] = rows / np.linalg.norm(rows, axis=1, keepdims=True)
    return x, q, spots


def test_fallen_back_waves_raise_words_the_others_no_longer_read(rmu):
    """Four records per list and 100 near-duplicates of a query in consecutive rows: the wave that meets them falls back, appends more than
    its slot holds, compacts and RAISES the query's shared word in the middle of the launch, while the waves of the other row chunks that
    hold the same query go on with the word they read at their first pair (option 0) or pick the new one up (option 1).  Same bits all
    ways, with the default capacity too; then with tombstones inside every cluster."""
    import torch
    x, q, spots = _clustered(95)
    idx = _index(rmu, x, "ip", 3, 256)
    qd = torch.from_numpy(q).cuda()
    try:
        for cap in (0, 4):
            for k in (10, 40):
                s, r, screened = three_ways(idx, qd, k, cap=cap)
                assert screened <= -3, screened                  # K' rows inside the band: the three queries are answered by the exact scan
                for i, rows in spots.items():
                    assert np.isin(r[i].cpu().numpy(), rows).all()
        dead = np.concatenate([rows[::3] for rows in spots.values()])
        assert idx.remove_rows(dead) == len(dead)
        for cap in (0, 4):
            s, r, _ = three_ways(idx, qd, 10, cap=cap)
            assert not np.isin(r.cpu().numpy(), dead).any()
            for i, rows in spots.items():
                assert np.isin(r[i].cpu().numpy(), rows).all()
    finally:
        idx.close()


def test_search_on_a_callers_stream(world):
    """One search ordered on the caller's stream (no host synchronisation inside the call) returns the bits of the default call, with
    either setting of the switch."""
    import torch
    idx, q = world("131100 default", "ip")
    s0, r0 = idx.search(q[:300], 10)
    st = torch.cuda.Stream()
    try:
        for refresh in (False, True):
            idx.set_screen_refresh(refresh)
            with torch.cuda.stream(st):
                qd = q[:300].clone()
                out = (torch.empty((300, 10), dtype=torch.float32, device="cuda"), torch.empty((300, 10), dtype=torch.int64, device="cuda"))
                st.synchronize()
                s1, r1 = idx.search(qd, 10, stream=st.cuda_stream, out=out)
                st.synchronize()
            assert torch.equal(r1, r0) and torch.equal(s1, s0), refresh
    finally:
        idx.set_screen_refresh(False)
