"""GPU: the 8-wave screening kernel on v_mfma_f32_16x16x32_f16 (csrc/scan_screen.hip).  Its accumulators reach the candidate path in the
MFMA's own layout and change owner only when something passes, so a wrong lane role shows as a wrong row id or a lost candidate: every case
compares the screened search, bit for bit, with the exact fp32 scan of the same index (set_screening(False)) and requires that the screen
answered (last_screened() != 0).  Batches over 128 queries take the 8-wave kernel; 129 and 257 leave partial query tiles, 41 003 rows a
partial last tile, 300 000 rows a ladder of seeded launches; k = 40 takes the DEEP slots."""
import numpy as np
import pytest

from oracle import oracle as O

pytestmark = pytest.mark.gpu

ROWS = (41_003, 300_000)
NQS = (129, 256, 257, 1024)
KS = (1, 10, 24, 32, 40)


@pytest.fixture(scope="module")
def rmu():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import ragmeup_amd
    from ragmeup_amd import _native
    _native.lib()                       # fails loudly if librmu.so is missing: there is no fallback
    return ragmeup_amd


@pytest.fixture(scope="module")
def data():
    x = O.make_corpus(300_000, seed=31)
    q, planted = O.make_queries(x[:41_003], 1024, seed=32)       # planted rows lie inside both corpora
    return x, q, planted


@pytest.fixture(scope="module")
def indexes(rmu, data):
    from ragmeup_amd import _native as N
    x, _, _ = data
    made = {}
    for n in ROWS:
        for name, metric in (("ip", N.METRIC_IP), ("l2", N.METRIC_L2SQ)):
            idx = rmu.FlatIndex(384, metric=metric)
            idx.set_screen_min_batch(1)          # RMU_OPT_SCREEN_MIN_NQ: 41 003 rows would otherwise go to the exact scan
            idx.add(x[:n])
            made[n, name] = idx
    yield made
    for idx in made.values():
        idx.close()


def screened_and_exact(idx, q, k):
    idx.set_screening(True)
    s, r = idx.search(q, k)
    screened = idx.last_screened()
    launches = idx.last_geometry()["launches"]
    idx.set_screening(False)
    s2, r2 = idx.search(q, k)
    assert idx.last_screened() == 0
    idx.set_screening(True)
    assert screened != 0, "expected the screening path"
    assert np.array_equal(r, r2) and np.array_equal(s, s2)
    return s, r, launches


@pytest.mark.parametrize("metric", ["ip", "l2"])
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("nq", NQS)
@pytest.mark.parametrize("n", ROWS)
def test_screened_equals_exact_scan(indexes, data, n, nq, k, metric):
    _, q, planted = data
    s, r, launches = screened_and_exact(indexes[n, metric], q[:nq], k)
    assert (r[:, 0] == planted[:nq]).all()
    if n == 300_000:
        assert launches >= 3, "expected a ladder of seeded launches"


@pytest.mark.parametrize("metric", ["ip", "l2"])
def test_every_lane_role_finds_its_planted_row(rmu, data, metric):
    """256 queries = 8 waves x 32 in-wave indices (0, 15, 16 and 31 among them); query (w, j) is row 32 * tile + (5 j + 3 + w) % 32 itself, so
    every in-wave index meets its best row at a different one of the 32 in-tile positions and every position is used in every wave."""
    from ragmeup_amd import _native as N
    x = data[0][:41_003].copy()
    rows = np.empty(256, np.int64)
    for w in range(8):
        for j in range(32):
            rows[32 * w + j] = 32 * (40 + 37 * (32 * w + j) % 1200) + (5 * j + 3 + w) % 32
    assert len(set(rows)) == 256 and {int(v) % 32 for v in rows[:32]} == set(range(32))
    q = x[rows].copy()
    idx = rmu.FlatIndex(384, metric=N.METRIC_L2SQ if metric == "l2" else N.METRIC_IP)
    idx.set_screen_min_batch(1)
    idx.add(x)
    for k in (1, 10):
        s, r, _ = screened_and_exact(idx, q, k)
        assert (r[:, 0] == rows).all()
    idx.close()


def test_near_duplicates_in_one_chunk_compact(rmu, data):
    """150 rows of rising similarity to one row, back to back: each beats everything before it, so the slots of the queries near that row
    (RMU_KS_CAP = 48 keys) fill and compact several times inside one chunk."""
    rng = np.random.default_rng(33)
    x = data[0][:41_003].copy()
    centre = x[777]
    a = np.linspace(0.3, 0.02, 150, dtype=np.float32)[:, None]
    dup = centre[None, :] + a * rng.standard_normal((150, 384)).astype(np.float32) / np.float32(np.sqrt(384.0))
    x[20_000:20_150] = dup / np.linalg.norm(dup, axis=1, keepdims=True)
    q = data[1][:257].copy()
    for qi in (0, 15, 16, 31, 100, 256):                             # queries of several lane roles sit on the cluster
        v = centre + 0.01 * rng.standard_normal(384).astype(np.float32) / np.float32(np.sqrt(384.0))
        q[qi] = v / np.linalg.norm(v)
    idx = rmu.FlatIndex(384)
    idx.set_screen_min_batch(1)
    idx.add(x)
    for k in (10, 32):
        s, r, _ = screened_and_exact(idx, q, k)
        assert set(r[0, :5]) <= set(range(20_100, 20_150)) | {777}
    idx.close()


def test_five_percent_tombstones(rmu, data):
    x, q, planted = data
    rng = np.random.default_rng(34)
    dead = np.unique(np.concatenate([rng.choice(41_003, 2050, replace=False), planted[:40]]))
    idx = rmu.FlatIndex(384)
    idx.set_screen_min_batch(1)
    idx.add(x[:41_003])
    idx.remove_rows(dead)
    s, r, _ = screened_and_exact(idx, q[:257], 10)
    assert not np.isin(r, dead).any()
    live = ~np.isin(planted[:257], dead)
    assert live.sum() > 150 and (r[live, 0] == planted[:257][live]).all()
    idx.close()
