"""GPU: the spill path of the screening ladder (RMU_OPT_SCREEN_SPILL; csrc/scan_screen.hip "Spill path", csrc/topk_merge.hip sift_kernel)
changes no answer.

Every case is searched three ways -- spill on (seeded 8-wave launches write passing lanes' accumulators out, the sift kernel files them),
spill off (appends inside the tile loop + merge, as before) and the exact fp32 scan -- and all three must return the same bits, ids and
scores; on and off must also re-run the same number of queries (last_screened()), and the K'-deep candidates of
rmu_index_screen_candidates must be equal with spill on and off.

Shapes: the smallest that run seeded 8-wave levels.  Below 64k rows the ladder's ratio is fixed at 8 (rmu_api.hip: ladder_bounds), so the
per-index options give 20 010 rows -> 288 / 2 496 / 20 010 (three levels, first range 256) and -- the smallest corpus with five levels --
131 100 rows -> 128 / 1 024 / 8 192 / 65 536 / 131 100 (ratio 2, first range 128); 70 000 rows cannot be cut into more than four.  Both
corpora end in a partial tile (20 010 = 625 tiles + 10 rows, 131 100 = 4 096 tiles + 28 rows).  Batches 129 / 256 / 300 / 1024: one
query in the second wave, one full workgroup, a part-filled second one, four query tiles; k = 1 .. 100: K' = 32, 40 (k > 24) and the deep
slots (k > 32)."""
import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu

LADDERS = {20_010: (8, 256, 3), 131_100: (2, 128, 5)}      # rows -> (ratio, first range, launches)
BATCHES = (129, 256, 300, 1024)
KS = (1, 10, 24, 32, 33, 100)
METRICS = ("ip", "cosine", "l2")


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
    ratio, first, _ = LADDERS[x.shape[0]]
    idx.set_ladder(ratio, first)
    idx.add(x)
    return idx


@pytest.fixture(scope="module")
def world(rmu):
    """Corpora, queries and indexes, made once and shared (no test modifies them; every test leaves the switches at their defaults)."""
    import torch
    made = {}

    def get(n, m):
        if (n, m) not in made:
            if n not in made:
                x = O.make_corpus(n, seed=71)
                qh = O.make_queries(x, 1024, seed=72)[0]
                made[n] = (x, qh, torch.from_numpy(qh).cuda())
            made[(n, m)] = _index(rmu, made[n][0], m)
        return made[(n, m)], made[n][2], made[n][1]

    yield get
    for key, v in made.items():
        if isinstance(key, tuple):
            v.close()


def three_ways(idx, q, k, launches, cap=0):
    """-> (scores, rows, last_screened) of the spill-on search, after checking it against spill off and the exact scan."""
    import torch
    out = {}
    try:
        for name in ("on", "off"):
            idx.set_screen_spill(name == "on", cap)
            s, r = idx.search(q, k)
            out[name] = (s, r, idx.last_screened())
            assert out[name][2] != 0, f"spill {name}: expected the screening path"
            assert idx.last_geometry()["launches"] == launches
    finally:
        idx.set_screen_spill(True, 0)
    idx.set_screening(False)
    try:
        se, re_ = idx.search(q, k)
        assert idx.last_screened() == 0
    finally:
        idx.set_screening(True)
    for name in ("on", "off"):
        s, r, _ = out[name]
        assert torch.equal(r, re_) and torch.equal(s, se), f"spill {name} differs from the exact scan at k = {k}"
    assert out["on"][2] == out["off"][2], (out["on"][2], out["off"][2])
    return out["on"]


def candidates_agree(idx, q_host):
    """rmu_index_screen_candidates (the true approximate top-K', no band): spill on == spill off, approximate scores and rows."""
    try:
        idx.set_screen_spill(True)
        on = idx.screen_candidates(q_host)
        idx.set_screen_spill(False)
        off = idx.screen_candidates(q_host)
    finally:
        idx.set_screen_spill(True, 0)
    assert np.array_equal(on[1], off[1])
    assert np.array_equal(on[0].view(np.int32), off[0].view(np.int32))
    assert (on[1][:, 0] >= 0).all()


@pytest.mark.parametrize("nq", BATCHES, ids=[f"{b}q" for b in BATCHES])
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("n", list(LADDERS))
def test_spill_on_off_and_exact_scan_agree(world, n, metric, nq):
    idx, q, _ = world(n, metric)
    for k in KS:
        three_ways(idx, q[:nq], k, LADDERS[n][2])


@pytest.mark.parametrize("nq", (300, 1024))
@pytest.mark.parametrize("metric", ("ip", "cosine"))
@pytest.mark.parametrize("n", list(LADDERS))
def test_candidates_are_equal(world, n, metric, nq):
    idx, _, qh = world(n, metric)
    candidates_agree(idx, qh[:nq])


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("n", list(LADDERS))
def test_four_records_per_list_fall_back_mid_launch(world, n, metric):
    """RMU_OPT_SCREEN_SPILL_CAP = 4: a wave's list takes its first few records, then the wave goes on through slow_path and its slots are
    emitted; the sift folds both."""
    idx, q, qh = world(n, metric)
    for nq in (300, 1024):
        for k in (10, 33, 100):
            three_ways(idx, q[:nq], k, LADDERS[n][2], cap=4)
    if metric != "l2":
        try:
            idx.set_screen_spill(True, 4)
            small = idx.screen_candidates(qh[:300])
        finally:
            idx.set_screen_spill(True, 0)
        full = idx.screen_candidates(qh[:300])
        assert np.array_equal(small[1], full[1]) and np.array_equal(small[0].view(np.int32), full[0].view(np.int32))


def test_forty_near_duplicates_in_one_tile(rmu):
    """40 rows within 1e-4 .. 1e-3 of a query direction in 40 CONSECUTIVE rows from a tile boundary of the last range on: every lane of the
    query's column passes in one tile (and a quarter of them in the next), the band holds more than K' = 32 rows, and the exact scan answers
    the query -- the same way with spill on, off, and with 4 records per list.  Queries 3, 150 and 290: group 0 of wave 0, group 1 of wave 4,
    the part-filled second workgroup."""
    import torch
    rng = np.random.default_rng(73)
    n = 20_010
    x = O.make_corpus(n, seed=74)
    q = O.make_corpus(300, seed=75)
    deficit = np.linspace(1e-4, 1e-3, 40)
    spots = {}
    for i, tile in ((3, 100), (150, 333), (290, 620)):
        rows = q[i][None, :] + np.sqrt(2.0 * deficit / 383.0)[:, None].astype(np.float32) * rng.standard_normal((40, 384)).astype(np.float32)
        spots[i] = np.arange(32 * tile, 32 * tile + 40)
        x[spots[i]] = rows / np.linalg.norm(rows, axis=1, keepdims=True)
    idx = _index(rmu, x)
    qd = torch.from_numpy(q).cuda()
    for cap in (0, 4):
        s, r, screened = three_ways(idx, qd, 10, 3, cap=cap)
        assert screened <= -3, screened
        for i, rows in spots.items():
            assert np.isin(r[i].cpu().numpy(), rows).all()
    candidates_agree(idx, q)
    idx.close()


def test_more_candidates_than_the_sifts_selection_array(rmu):
    """1 500 consecutive rows of the last range within 1e-3 of one query: all of them pass the seeded threshold, the query's candidates
    outgrow the 1024 keys the sift ranks in LDS, and its first wave folds them through the stream merge instead.  Same answers, same K'-deep
    candidates."""
    import torch
    rng = np.random.default_rng(78)
    x = O.make_corpus(20_010, seed=79)
    q = O.make_corpus(300, seed=80)
    rows = q[7][None, :] + np.sqrt(2.0 * rng.uniform(1e-4, 1e-3, 1500) / 383.0)[:, None].astype(np.float32) * rng.standard_normal((1500, 384)).astype(np.float32)
    x[5000:6500] = rows / np.linalg.norm(rows, axis=1, keepdims=True)
    idx = _index(rmu, x)
    qd = torch.from_numpy(q).cuda()
    for k in (10, 100):
        s, r, screened = three_ways(idx, qd, k, 3)
        assert screened < 0
        assert ((r[7] >= 5000) & (r[7] < 6500)).all()
    candidates_agree(idx, q)
    idx.close()


def test_spill_with_tombstones(rmu):
    """Every third row of a first search's results deleted: the three searches still agree, and none returns a deleted row."""
    import torch
    x = O.make_corpus(20_010, seed=76)
    q = torch.from_numpy(O.make_queries(x, 300, seed=77)[0]).cuda()
    idx = _index(rmu, x)
    _, r0, _ = three_ways(idx, q, 10, 3)
    dead = np.unique(r0.cpu().numpy().reshape(-1))[::3]
    assert idx.remove_rows(dead) == len(dead)
    for cap in (0, 4):
        _, r1, _ = three_ways(idx, q, 10, 3, cap=cap)
        assert not np.isin(r1.cpu().numpy(), dead).any()
    idx.close()


def test_search_on_a_callers_stream(world):
    """One spilled search ordered on the caller's stream (no host synchronisation inside the call) returns the bits of the default call."""
    import torch
    idx, q, _ = world(131_100, "ip")
    s0, r0 = idx.search(q[:300], 10)
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        qd = q[:300].clone()
        out = (torch.empty((300, 10), dtype=torch.float32, device="cuda"), torch.empty((300, 10), dtype=torch.int64, device="cuda"))
        st.synchronize()
        s1, r1 = idx.search(qd, 10, stream=st.cuda_stream, out=out)
        st.synchronize()
    assert torch.equal(r1, r0) and torch.equal(s1, s0)
