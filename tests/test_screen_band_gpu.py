"""GPU: band seeding of the screening ladder (RMU_OPT_SCREEN_BAND; csrc/scan_screen.hip header "Band seeding") changes no answer.

Every case is searched three ways -- band on, band off (the K'-th best alone seeds the thresholds, as before), and the exact fp32 scan --
and all three must return the same bits; band on and off must also re-run the same number of queries (last_screened()).  The ladder is
pinned to ratio 3 / first range 256: 70 000 rows -> 1 088 / 8 736 / 70 000 (two seeded launches), 300 000 rows -> 1 536 / 12 480 / 99 968 /
300 000 (three), so every merge form that seeds a launch is behind these answers: the first merge's unsorted mode, K' = 32 / 40 (k <= 32,
the 1024-key selection) and K' = 41 / 120 (the 3072-key selection), in the 8-wave and the one-tile 4-wave scan."""
import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu

ROWS = {70_000: 3, 300_000: 4}                       # rows -> launches of the ladder at ratio 3 / first 256
BATCHES = [(130, False), (300, False), (1024, False), (5, True), (100, True)]      # (queries, forced through the one-tile 4-wave kernel)
KS = (1, 10, 24, 25, 32, 33, 100)
METRICS = ("ip", "cosine", "l2")


@pytest.fixture(scope="module")
def rmu():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import ragmeup_amd
    from ragmeup_amd import _native
    _native.lib()
    return ragmeup_amd


@pytest.fixture(scope="module")
def world(rmu):
    """Corpora, queries and indexes, made once and shared (nothing here is modified by a test)."""
    import torch
    from ragmeup_amd import _native as N
    metric = {"ip": N.METRIC_IP, "cosine": N.METRIC_COSINE, "l2": N.METRIC_L2SQ}
    made = {}

    def get(n, m):
        if (n, m) not in made:
            if n not in made:
                x = O.make_corpus(n, seed=61)
                made[n] = (x, torch.from_numpy(O.make_queries(x, 1024, seed=62)[0]).cuda())
            idx = rmu.FlatIndex(384, metric=metric[m])
            idx.set_ladder(3, 256)
            idx.add(made[n][0])
            made[(n, m)] = idx
        return made[(n, m)], made[n][1]

    yield get
    for key, v in made.items():
        if isinstance(key, tuple):
            v.close()


def three_ways(idx, q, k, launches=None):
    """-> (scores, rows, last_screened) of the band-on search, after checking it against band off and the exact scan."""
    import torch
    out = {}
    for name in ("on", "off"):
        idx.set_screen_band(name == "on")
        s, r = idx.search(q, k)
        out[name] = (s, r, idx.last_screened())
        assert out[name][2] != 0, f"band {name}: expected the screening path"
        if launches is not None:
            assert idx.last_geometry()["launches"] == launches
    idx.set_screen_band(True)
    idx.set_screening(False)
    se, re_ = idx.search(q, k)
    assert idx.last_screened() == 0
    idx.set_screening(True)
    for name in ("on", "off"):
        s, r, _ = out[name]
        assert torch.equal(r, re_) and torch.equal(s, se), f"band {name} differs from the exact scan at k = {k}"
    assert out["on"][2] == out["off"][2], (out["on"][2], out["off"][2])
    return out["on"]


@pytest.mark.parametrize("nq,one_tile", BATCHES, ids=[f"{b}q" + ("-4wave" if t else "") for b, t in BATCHES])
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("n", list(ROWS))
def test_band_on_off_and_exact_scan_agree(world, n, metric, nq, one_tile):
    idx, q = world(n, metric)
    idx.set_screen_min_batch(1 if one_tile else 0)
    try:
        for k in KS:
            three_ways(idx, q[:nq], k, ROWS[n])
    finally:
        idx.set_screen_min_batch(0)


def test_crowded_bands_are_rerun_alike(rmu):
    """40 rows within 1e-4 .. 1e-3 of each of 20 query directions: at k = 10 the band (2 EPS ~ 1e-3 for unit vectors) holds more than K' = 32
    rows, the sufficiency test fails with and without the band, and the exact scan answers those queries."""
    import torch
    rng = np.random.default_rng(63)
    x = O.make_corpus(70_000, seed=64)
    q = O.make_corpus(300, seed=65)
    spots = rng.permutation(70_000)[:20 * 40].reshape(20, 40)               # spread over all three row ranges
    deficit = np.linspace(1e-4, 1e-3, 40)
    for i in range(20):
        rows = q[i][None, :] + np.sqrt(2.0 * deficit / 383.0)[:, None].astype(np.float32) * rng.standard_normal((40, 384)).astype(np.float32)
        x[spots[i]] = rows / np.linalg.norm(rows, axis=1, keepdims=True)
    idx = rmu.FlatIndex(384)
    idx.set_ladder(3, 256)
    idx.add(x)
    s, r, screened = three_ways(idx, torch.from_numpy(q).cuda(), 10, 3)
    assert screened <= -20, screened
    assert np.isin(r[:20].cpu().numpy(), spots).all()
    idx.close()


def test_band_with_tombstones(rmu):
    """Every third row of a first search's results deleted: the three searches still agree, and none returns a deleted row."""
    import torch
    x = O.make_corpus(70_000, seed=66)
    q = torch.from_numpy(O.make_queries(x, 300, seed=67)[0]).cuda()
    idx = rmu.FlatIndex(384)
    idx.set_ladder(3, 256)
    idx.add(x)
    _, r0, _ = three_ways(idx, q, 10, 3)
    dead = np.unique(r0.cpu().numpy().reshape(-1))[::3]
    assert idx.remove_rows(dead) == len(dead)
    _, r1, _ = three_ways(idx, q, 10, 3)
    assert not np.isin(r1.cpu().numpy(), dead).any()
    idx.close()
