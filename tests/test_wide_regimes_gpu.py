"""The wide exact scan (`scan_wide_kernel`: rows of 769..3072 dimensions and every RMU_OPT_WIDE_SCAN search) held to its fmaf chain, bit
for bit, in every geometry.

tests/wide_regimes.py restates rmu_wide_plan and lists the cases: every configuration with 1, 2 and 3 tiles per workgroup at the widths
832, 1024 (with and without padding columns), 1536 and 3072, both block-map branches, 1..4 query tiles of the k > 32 form, every nq / k
boundary from both sides, and the corpora that drive the selection machinery (floods of bit-identical best rows sized for the wide slot
depths, rising / falling scores, an all-zero query, deleted rows) -- and the narrow corpora of tests/exact_regimes.py through the wide
kernel, against the references that module computes for scan_topk_kernel.  The reference is that module's chain (oracle_chain_scores,
checked against a numpy twin on the CPU) over the restated images.  Here every case must
  * have run the planned regime: FlatIndex.last_geometry() == the planned grid and LDS bytes, in one launch;
  * return the reference's score BITS and row ids.  There is no tolerance and no tie rule in this file: equal scores are ordered by row.
Two tests place a flood where the `>=` of the shared bound decides the answer and no race hides it: five tiles per workgroup in one
launch (k <= 32) and the last level of the threshold ladder (k > 32); a filter that passes only v > bound fails both.
The queries of every case are a prefix of ONE batch per family, so a query's answer is also compared across the batch sizes (and wq) it
travels with.  One index per family is grown by `add` through the ascending row counts.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import exact_regimes as E
from tests import wide_regimes as W

pytestmark = pytest.mark.gpu

FAMILIES = W.families()


@pytest.fixture(scope="module")
def rmu():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import ragmeup_amd
    from ragmeup_amd import _native
    _native.lib()
    return ragmeup_amd


def _report(failures):
    assert not failures, f"{len(failures)} mismatches:\n" + "\n".join(failures[:12])


@pytest.mark.parametrize("family", list(FAMILIES), ids=["-".join(map(str, f)) for f in FAMILIES])
def test_every_case_runs_its_regime_and_returns_the_chain_bits(rmu, family):
    """IP: scores and rows equal expected_topk(chain).  COSINE: the chain over the restated images of rows and queries (k_row_norm).
    Families of 768 dimensions and less run the wide kernel through RMU_OPT_WIDE_SCAN."""
    failures, checked = W.run_family(rmu.FlatIndex, family, FAMILIES[family])
    assert checked == len(FAMILIES[family])
    _report(failures)


def _steps(dim):
    """(n, nq, k) of one case per RT at its deepest tile class that the width runs"""
    out = []
    for rt, nq, k in ((32, 65, 32), (64, 33, 33), (128, 32, 32)):
        rows = W.class_rows(rt)
        out.append((rows["t3"] if rows["t3"] <= W.rows_max(W.WIDE_DIMS[dim]) else rows["t2"], nq, k))
    return sorted(out)


def _check(idx, ref, n, nq, k, alive, failures, tag, q=None):
    p = W.plan_wide(n, nq, k, ref.dpad)
    s, r = idx.search(ref.q[:nq] if q is None else q, k)
    if q is not None:
        s, r = s.cpu().numpy(), r.cpu().numpy()
    g = W.geometry_mismatch(idx.last_geometry(), p)
    if g:
        failures.append(f"{tag} n={n} nq={nq} k={k}: {g}")
    m = W.mismatch(s, r, *ref.topk(n, nq, k, alive))
    if m:
        failures.append(f"{tag} n={n} nq={nq} k={k} [{p['config']}]: {m}")
    return s, r


@pytest.mark.parametrize("dim", [769, 1024, 3072])
def test_removed_rows_are_absent_and_nothing_else_moves(rmu, dim):
    """holes: the first and the last row of a tile, a whole tile, a whole chunk and the best row of every query are deleted (at the
    geometry of each RT in turn); the reference drops the same rows."""
    steps = _steps(dim)
    ref = W.Reference(dim, "random", "ip", [W.Case(dim, "random", "ip", n, nq, k) for n, nq, k in steps])
    idx = rmu.FlatIndex(dim)
    idx.set_screening(False)
    alive = np.ones(ref.n_max, bool)
    failures, have = [], 0
    for n, nq, k in steps:
        idx.add(ref.x[have:n])
        have = n
        top1 = ref.topk(n, nq, 1, alive)[1][:, 0]
        dead = W.holes(W.plan_wide(n, nq, k, ref.dpad), n, top1[top1 >= 0])
        dead = dead[alive[dead]]
        assert idx.remove_rows(dead) == dead.size
        alive[dead] = False
        for kk in (k, 1):
            _, r = _check(idx, ref, n, nq, kk, alive, failures, "holes")
            assert not np.isin(r, np.nonzero(~alive)[0]).any(), "a removed row was returned"
    idx.close()
    _report(failures)


@pytest.mark.parametrize("dim", [1024, 769])
def test_host_and_device_queries_alone_and_in_a_batch_return_the_same_bits(rmu, dim):
    """The same queries alone and inside batches that change wq (1 -> 2 -> 4) and the number of query tiles -- at k = 33 w2_k1 with 1, 1, 1
    and 3 query tiles -- from host memory and from device memory (1024: dim == dpad, the device form reads the caller's buffer in place;
    769: padding columns), and an all-zero batch: rows 0..k-1, score bits 0."""
    import torch
    n = W.class_rows(32)["t3"]
    shapes = tuple((nq, k) for k in (32, 33) for nq in (5, 32, 33, 129))
    ref = W.Reference(dim, "random", "ip", [W.Case(dim, "random", "ip", n, nq, k) for nq, k in shapes])
    idx = rmu.FlatIndex(dim)
    idx.set_screening(False)
    idx.add(ref.x[:n])
    failures, got = [], {}
    qd = torch.from_numpy(ref.q).cuda()
    for nq, k in shapes:
        got[(nq, k)] = _check(idx, ref, n, nq, k, None, failures, "host")
        sd, rd = _check(idx, ref, n, nq, k, None, failures, "device", q=qd[:nq])
        if W.mismatch(sd, rd, *got[(nq, k)]):
            failures.append(f"nq={nq} k={k}: device queries and host queries differ: " + W.mismatch(sd, rd, *got[(nq, k)]))
    for k in (32, 33):
        for nq in (32, 33, 129):                               # the first five queries: alone, with 32, 33 and 129
            m = W.mismatch(got[(nq, k)][0][:5], got[(nq, k)][1][:5], *got[(5, k)])
            if m:
                failures.append(f"k={k}: five queries alone and in a batch of {nq} differ: {m}")
    for nq, k in ((1, 1), (32, 32), (33, 33), (129, 112)):
        s, r = idx.search(np.zeros((nq, dim), np.float32), k)
        if not ((W.bits(s) == 0).all() and (r == np.arange(k)[None, :]).all()):
            failures.append(f"zero queries nq={nq} k={k}: rows {r[0][:8]}..., bits {W.bits(s)[0][:4]}")
    idx.close()
    _report(failures)


def test_fewer_live_rows_than_k(rmu):
    """n in {1, 31, 33, 129} with k in {1, 32, 33, 112}: the live rows in order, bit for bit, then (-inf, -1)"""
    dim, nq = 1024, 5
    x, q = W.corpus("random", dim, 4000)
    idx = rmu.FlatIndex(dim)
    idx.set_screening(False)
    failures, have = [], 0
    for n in (1, 31, 33, 129):
        idx.add(x[have:n])
        have = n
        scores = W.chain(q[:nq], x[:n], dim)
        for k in (1, 32, 33, 112):
            s, r = idx.search(q[:nq], k)
            g = W.geometry_mismatch(idx.last_geometry(), W.plan_wide(n, nq, k, dim))
            m = W.mismatch(s, r, *W.expected_topk(scores, None, k))
            failures += [f"n={n} k={k}: {v}" for v in (g, m) if v]
            if k > n and not ((r[:, n:] == -1).all() and np.isneginf(s[:, n:]).all()):
                failures.append(f"n={n} k={k}: the tail is not (-inf, -1)")
    idx.close()
    _report(failures)


def test_the_pin_tells_the_kernel_s_k_order_from_the_natural_one(rmu):
    """The same products summed in the order k = 0, 1, 2, ... are NOT what the kernel returns: for most (query, rank) pairs the
    natural-order score of the returned row has other bits, while the chain's has the returned bits."""
    dim, n, nq, k = 1024, W.class_rows(32)["t2"], 65, 32
    x, q = W.corpus("random", dim, n)
    idx = rmu.FlatIndex(dim)
    idx.set_screening(False)
    idx.add(x)
    s, r = idx.search(q[:nq], k)
    idx.close()
    live = [i for i in range(nq) if i != W.ZERO_QUERY]
    nat = np.take_along_axis(E.cflat.chain_scores(q[:nq], x, dim, natural=True), r, axis=1)
    own = np.take_along_axis(W.chain(q[:nq], x, dim), r, axis=1)
    assert np.array_equal(W.bits(own), W.bits(s))
    assert (W.bits(nat) != W.bits(s))[live].mean() > 0.5


def test_rows_that_meet_a_shared_bound_equal_to_their_score_are_kept(rmu):
    """Five tiles per workgroup: the lowest rows of a flood are the last rows their workgroup scans, three tiles after another
    workgroup has published the flood's score as the shared bound (wide_regimes.LATE).  They equal the bound and belong to the answer."""
    x, q, floods = W.late_corpus()
    dpad = W.WIDE_DIMS[W.LATE_DIM]
    scores = W.chain_blocked(q, x, dpad)
    idx = rmu.FlatIndex(W.LATE_DIM, capacity_hint=x.shape[0])
    idx.set_screening(False)
    failures, have = [], 0
    for i, (rt, nq, k) in enumerate(W.LATE):
        n = W.late_rows(rt)
        idx.add(x[have:n])
        have = n
        p = W.plan_wide(n, nq, k, dpad)
        es, er = W.expected_topk(scores[:nq, :n], None, k)
        assert np.array_equal(er[i, :k], floods[i][:k]) and len(set(W.bits(es[i]).tolist())) == 1       # what the corpus is built for
        s, r = idx.search(q[:nq], k)
        g, m = W.geometry_mismatch(idx.last_geometry(), p), W.mismatch(s, r, es, er)
        failures += [f"n={n} nq={nq} k={k} [{p['config']}, {p['tiles_per_chunk']} tiles per workgroup]: {v}" for v in (g, m) if v]
    idx.close()
    _report(failures)


@pytest.mark.parametrize("env", [{"RMU_NT": "0"}, {"RMU_NO_SHARED_THR": "1"}], ids=["no_nontemporal_stream", "no_shared_thresholds"])
def test_the_switched_forms_return_the_chain_bits(env):
    """The forms reached only through environment switches read at first use -- the plain (not non-temporal) w1_k0 and w2_k0, and
    share_thr = 0 -- in a fresh interpreter each, against the same expectations (tests/wide_variant_driver.py)."""
    here = os.path.dirname(os.path.abspath(__file__))
    out = subprocess.run([sys.executable, os.path.join(here, "wide_variant_driver.py")], env=dict(os.environ, RMU_TUNING="1", **env),
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    res = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    assert res["checked"] == len(W.variant_cases())
    if "RMU_NT" in env:
        assert {"w1_k0", "w2_k0"} <= set(res["configs"]) and not any(c.endswith("_nt") for c in res["configs"])
    else:
        assert {"w1_k0_nt", "w2_k0_nt"} <= set(res["configs"])
    _report(res["failures"])


def test_the_ladder_meets_bounds_equal_to_the_scores_still_to_come(rmu):
    """k > 32 over 262 144 + 77 rows: the threshold ladder, every level a launch of the wide kernel with a row0 and shared thresholds
    seeded from the levels before it.  Floods of 113 and 34 bit-identical best rows lie across the ends of the first two levels
    (deep_bounds: 16 384, 65 536, n), so a level's k-th best seeds the next one with a bound EQUAL to the scores still to come.  A third
    flood is spread inside the last level: its lowest rows are scanned long after another workgroup has published their score as the
    shared bound, and belong to the answer (wide_regimes.ladder_floods)."""
    x, q, floods = W.ladder_corpus()
    n, dpad = W.LADDER_N, W.WIDE_DIMS[W.LADDER_DIM]
    bounds = W.deep_bounds(n)
    assert bounds == [16_384, 65_536, n] and [int(f[len(f) // 2]) for f in floods[:2]] == bounds[:2]
    scores = W.chain_blocked(q, x, dpad)
    idx = rmu.FlatIndex(W.LADDER_DIM, capacity_hint=n)
    idx.set_screening(False)
    idx.add(x)
    failures = []
    for k in (33, 112):
        es, er = W.expected_topk(scores, None, k)
        for i, rows in enumerate(floods):                          # what the corpus is built for: the answer is the flood's lowest rows
            kk = min(k, rows.size)
            assert np.array_equal(er[i, :kk], rows[:kk]) and len(set(W.bits(es[i, :kk]).tolist())) == 1
        s, r = idx.search(q, k)
        if idx.last_geometry()["launches"] <= 1:
            failures.append(f"k={k}: the ladder did not run ({idx.last_geometry()})")
        m = W.mismatch(s, r, es, er)
        if m:
            failures.append(f"ladder k={k}: {m}")
    idx.close()
    _report(failures)
