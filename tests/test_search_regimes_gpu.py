"""Every re-run class of the screened search against the fp64 oracle, on both sides of each class boundary.

tests/search_regimes.py restates the dispatch of `rmu_index_search` and builds, for each case, a batch whose number of flagged
queries is known without the library: certain-fail queries (a duplicate cluster of their own each, or an fp16 overflow) among
certain-pass ones (fp64 margin s_k - s_K' >= 5 EPS).  tests/test_search_regimes_cpu.py guards the restated constants and re-derives
the verdicts of the small cases.  Here, per case:
  1. control: the background queries alone must not flag anything (a wrong margin rule fails HERE, loudly, not as a miscount);
  2. the full batch: last_screened() == -c exactly;
  3. every query, flagged or not, against the oracle (run at k + 4) under the tie rule; the tied ones return the ascending ids of
     their OWN cluster -- a permuted scatter shows here.  A tied query that nobody re-runs keeps a RIGHT answer (the re-score ranks
     the K' lowest ids of its cluster as the exact scan does), so from two flagged queries on a case also holds an fp16-overflow
     query and graded clusters (tests/search_regimes.py), whose answers are wrong unless the exact scan replaces them;
  4. bit-identical ids and scores with the screening switched off;
  5. the same call again: same bits, same count (a stale flag, list or threshold word), then a batch that flags nothing reports > 0.
The 8192-query cut (output offsets, the per-block drain, the count summed over blocks, a short last block of another class) has
its own two requests, through host arrays, device tensors, a caller stream, the exact scan and the deep ladder.
"""
import numpy as np
import pytest

from tests import search_regimes as R
from tests.helpers import assert_topk_parity

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rmu():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import ragmeup_amd
    from ragmeup_amd import _native
    _native.lib()                       # fails loudly if librmu.so is missing: there is no fallback
    return ragmeup_amd


def _index(rmu, case, b):
    from ragmeup_amd import _native as N
    # the builder's precondition, for the cases the CPU file does not re-derive as well: every verdict rests on a margin of >= 5 EPS
    assert (b.margins >= R.MARGIN_EPS).all(), f"{case.id}: margins down to {b.margins.min():.2f} EPS"
    idx = rmu.FlatIndex(384, metric={"ip": N.METRIC_IP, "cosine": N.METRIC_COSINE, "l2": N.METRIC_L2SQ}[case.metric])
    idx.add(b.x)
    if b.dead.size:
        idx.remove_rows(b.dead)
    idx.set_screen_min_batch(case.min_batch)
    return idx


def _clean_batch_is_clean(idx, case, b, what):
    """the certain-pass queries of the case alone (the spare ones when every query is flagged): screened, nothing re-run"""
    bg = b.q[b.kinds == "b"]
    idx.set_screen_min_batch(1)                      # (this batch is narrower than the case: screen it whatever its size)
    idx.search(bg if bg.shape[0] else b.spare, case.k, case.row_base)
    got = idx.last_screened()
    idx.set_screen_min_batch(case.min_batch)
    assert got > 0, f"{what}: a batch of certain-pass queries reports {got}"


def _oracle_subset(case, b):
    """every query, except over the 270 000-row corpora: there every flagged query, its neighbours on both sides, both ends, the rows
    around a block cut and a seeded handful of the rest"""
    if case.n < R.DEEP_N:
        return np.arange(case.nb)
    rng = np.random.default_rng(case.nb + case.count)
    near = np.concatenate([b.flagged - 1, b.flagged, b.flagged + 1, [0, case.nb - 1], rng.permutation(case.nb)[:12]])
    return np.unique(near[(near >= 0) & (near < case.nb)])


def _check_against_oracle(case, b, s, r, sub):
    """s, r: what the library returned for the whole request (row ids without the row_base)"""
    sc = -s if case.metric == "l2" else s             # the L2 index reports squared distances, the oracle -(distance)
    os_, or_ = R.oracle_topk(b.q[sub], b.x, case.k + 4, case.metric, alive=b.alive if b.dead.size else None,
                             budget=1 << (27 if case.n >= R.DEEP_N else 25), rep=b.rep)
    plain = b.kinds[sub] != "o"
    scale = max(1.0, float(np.abs(os_[plain]).max())) if case.metric == "l2" else 1.0      # |q|^2 + |x|^2 up to ~5; unit scores otherwise
    assert_topk_parity(sc[sub][plain], r[sub][plain], os_[plain], or_[plain], score_tol=1e-4 * scale, tie_tol=1e-6 * scale)
    for j in np.nonzero(~plain)[0]:                   # the overflowing query: scores of |q| ~ 50 000, the bars scale with them
        big = max(1.0, float(np.abs(os_[j]).max()))
        assert_topk_parity(sc[sub][j:j + 1], r[sub][j:j + 1], os_[j:j + 1], or_[j:j + 1], score_tol=1e-4 * big, tie_tol=1e-6 * big)
    for p, ids in b.expect.items():                   # ties resolve to the ascending live ids of the query's own cluster
        assert np.array_equal(r[p], ids), f"query {p}: {r[p]} instead of its cluster {ids}"
    order = np.diff(s, axis=1)
    assert (order >= 0).all() if case.metric == "l2" else (order <= 0).all()


@pytest.mark.parametrize("case", R.CASES, ids=[c.id for c in R.CASES])
def test_rerun_class_against_the_oracle(rmu, case):
    b = R.build(case)
    idx = _index(rmu, case, b)
    k, want = case.k, (-case.count if case.count else 1)
    if case.n >= R.DEEP_N and k > 32:
        assert R.screen_kp(k) > R.KS_CAP - 8               # the deep screen: K' beyond the 48-key slots

    _clean_batch_is_clean(idx, case, b, "control")                                        # 1

    s, r = idx.search(b.q, k, case.row_base)                                              # 2
    got = idx.last_screened()
    print(f"{case.id}: class {case.classes[0]}, last_screened {got}, expected {'> 0' if want > 0 else want}")
    assert (got > 0) if want > 0 else (got == want), f"last_screened() = {got}, {case.count} certain-fail queries in the batch"
    assert (r >= case.row_base).all()
    _check_against_oracle(case, b, s, r - case.row_base, _oracle_subset(case, b))         # 3

    idx.set_screening(False)                                                              # 4
    s2, r2 = idx.search(b.q, k, case.row_base)
    assert idx.last_screened() == 0
    idx.set_screening(True)
    diff = np.nonzero((r2 != r).any(axis=1) | (s2 != s).any(axis=1))[0]
    assert diff.size == 0, f"queries {diff[:20]} differ from the exact scan (flagged: {b.flagged[:20]})"

    s3, r3 = idx.search(b.q, k, case.row_base)                                            # 5
    assert idx.last_screened() == got and np.array_equal(r3, r) and np.array_equal(s3, s)
    _clean_batch_is_clean(idx, case, b, "after a flagged batch")
    idx.close()


# ---- requests of more than one query block ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.BLOCK_CASES, ids=[c.id for c in R.BLOCK_CASES])
def test_query_blocks_on_the_screened_path(rmu, case):
    import torch
    b = R.build(case)
    idx = _index(rmu, case, b)
    k = case.k
    assert [R.path(case.n, nbb, k, 384, min_nq=case.min_batch) for _, nbb in R.blocks(case.nb)] == ["screen", "screen"]
    _clean_batch_is_clean(idx, case, b, "control")
    # host arrays
    s, r = idx.search(b.q, k)
    got = idx.last_screened()
    print(f"{case.id}: classes {case.classes}, last_screened {got}, expected {-case.count}")
    assert got == -case.count, f"last_screened() = {got}: the blocks flag {case.c}"        # the SUM over the blocks
    assert set(R.BLOCK_SEAM) <= set(range(case.nb))
    _check_against_oracle(case, b, s, r, np.arange(case.nb))                                # (every row: the seam rows among them)
    s3, r3 = idx.search(b.q, k)
    assert idx.last_screened() == got and np.array_equal(r3, r) and np.array_equal(s3, s)
    # the exact scan, cut the same way
    idx.set_screening(False)
    s2, r2 = idx.search(b.q, k)
    assert idx.last_screened() == 0
    idx.set_screening(True)
    diff = np.nonzero((r2 != r).any(axis=1) | (s2 != s).any(axis=1))[0]
    assert diff.size == 0, f"queries {diff[:20]} differ from the exact scan (flagged: {b.flagged})"
    # device tensors, complete on return
    qd = torch.from_numpy(b.q).cuda()
    sd, rd = idx.search(qd, k)
    assert idx.last_screened() == got
    assert np.array_equal(rd.cpu().numpy(), r) and np.array_equal(sd.cpu().numpy(), s)
    # device tensors on a caller stream: the last block is not drained, its count is not reported (include/rmu.h) -- results and != 0 only
    st = torch.cuda.Stream()
    out_s = torch.full((case.nb, k), float("nan"), dtype=torch.float32, device="cuda")
    out_r = torch.full((case.nb, k), -7, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    so, ro = idx.search(qd, k, stream=st.cuda_stream, out=(out_s, out_r))
    st.synchronize()
    assert idx.last_screened() != 0
    assert np.array_equal(ro.cpu().numpy(), r) and np.array_equal(so.cpu().numpy(), s)
    _clean_batch_is_clean(idx, case, b, "after the caller-stream search")
    idx.close()


@pytest.mark.parametrize("nq", [c.nb for c in R.BLOCK_CASES])
def test_query_blocks_on_the_deep_ladder(rmu, nq):
    """k = 40 over 270 000 rows with the screening off: each block runs the exact ladder over the corpus ranges, the thread's
    workspace is reused between blocks.  The request repeats 1088 distinct queries: every row must equal its first occurrence
    bit for bit (a result written at a wrong offset, or a block computed on stale workspace, cannot), and the first occurrence of
    every query and the rows around the cut are compared with the oracle."""
    k = 40
    pool = R._pool("deep", R.DEEP_ROWS, R.DEEP_CLUSTERS * R.DEEP_PER_CLUSTER, k)
    m = pool["q"].shape[0]
    q = np.ascontiguousarray(pool["q"][np.arange(nq) % m])
    assert [R.path(R.DEEP_ROWS, nbb, k, 384, screening=False) for _, nbb in R.blocks(nq)] == ["deep_ladder", "deep_ladder"]
    idx = rmu.FlatIndex(384)
    idx.add(pool["x"])
    idx.set_screening(False)
    s, r = idx.search(q, k)
    assert idx.last_screened() == 0 and idx.last_geometry()["launches"] >= 2
    first = np.arange(nq) % m
    assert np.array_equal(r, r[first]) and np.array_equal(s, s[first])
    sub = np.unique(np.concatenate([np.arange(m), R.BLOCK_SEAM, [nq - 2, nq - 1]]))       # every distinct query once, and the cut
    assert_topk_parity(s[sub], r[sub], *R.oracle_topk(q[sub], pool["x"], k + 4, budget=1 << 27))
    idx.close()


# ---- two more call sites of the same code --------------------------------------------------------------------------------------------
def test_search_mmr_over_a_batch_with_flagged_queries(rmu):
    """rmu_index_search_mmr runs the same search: 1024 queries, 40 of them flagged (mid class), fetch_k = 20, k = 4"""
    case = R.Case("mmr-nb1024-c40-mid", 1024, (40,), k=20)
    b = R.build(case)
    idx = _index(rmu, case, b)
    s, r = idx.search(b.q, 20)
    assert idx.last_screened() == -40
    for p, ids in b.expect.items():                     # the flagged queries' candidates are their clusters
        assert np.array_equal(r[p], ids)
    assert_topk_parity(s, r, *R.oracle_topk(b.q, b.x, 24, rep=b.rep))
    pos = idx.mmr(b.q, r, 4).astype(np.int64)
    rows, sc = idx.search_mmr(b.q, 20, 4)
    assert np.array_equal(rows, np.take_along_axis(r, pos, axis=1)) and np.array_equal(sc, np.take_along_axis(s, pos, axis=1))
    for p, ids in b.expect.items():
        assert set(rows[p].tolist()) <= set(ids.tolist())
    idx.close()


@pytest.mark.parametrize("cid", ["ip-nb1024-c33-mid", "ip-nb1024-c129-whole"])
def test_caller_stream_with_device_outputs(rmu, cid):
    """The re-run decision is taken on the device: on a caller stream with device buffers nothing waits on the host, and the
    gathered classes scatter into the caller's tensors."""
    import torch
    from ragmeup_amd import _native as N
    case = next(c for c in R.CASES if c.id == cid)
    b = R.build(case)
    idx = _index(rmu, case, b)
    st = torch.cuda.Stream()
    qd = torch.from_numpy(b.q).cuda()
    out_s = torch.full((case.nb, case.k), float("nan"), dtype=torch.float32, device="cuda")
    out_r = torch.full((case.nb, case.k), -7, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    N.check(N.lib().rmu_index_search(idx._h, qd.data_ptr(), case.nb, case.k, N.F_Q_DEVICE | N.F_OUT_DEVICE, 0, out_s.data_ptr(),
                                     out_r.data_ptr(), st.cuda_stream), "rmu_index_search")
    st.synchronize()
    assert idx.last_screened() != 0
    s, r = out_s.cpu().numpy(), out_r.cpu().numpy()
    _check_against_oracle(case, b, s, r, np.arange(case.nb))
    idx.set_screening(False)
    s2, r2 = idx.search(b.q, case.k)
    assert idx.last_screened() == 0 and np.array_equal(r2, r) and np.array_equal(s2, s)
    idx.close()
