"""The exact fp32 scan (`scan_topk_kernel`) held to its fmaf chain, bit for bit, in every geometry.

tests/exact_regimes.py restates the planner, the chain (oracle/flat_search.c: oracle_chain_scores, checked against a numpy twin on the
CPU), the image kernels of COSINE and L2 indexes and the merge's last L2 step, and lists CASES: every (padded width x configuration) with
1, 2, 3 and 4 tiles per workgroup, both block-map branches with one and two query tiles, every nq / k boundary from both sides, and the
corpora that drive the selection machinery (rising / falling scores, floods of bit-identical best rows, an all-zero query, deleted
rows).  Here every case must
  * have run the planned regime: FlatIndex.last_geometry() == the planned grid and LDS bytes, in one launch;
  * return the reference's score BITS and row ids.  There is no tolerance and no tie rule in this file: equal scores are ordered by row.
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

pytestmark = pytest.mark.gpu

FAMILIES = E.families()


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
    """IP: scores and rows equal expected_topk(chain).  COSINE and L2: the chain over the restated images (k_row_norm; k_l2_aug_rows,
    k_l2_aug_queries) and, for L2, the restated merge step max(|q|^2 - s, 0)."""
    failures, checked = E.run_family(rmu.FlatIndex, family, FAMILIES[family])
    assert checked == len(FAMILIES[family])
    _report(failures)


def _steps(dim):
    """(n, nq, k) of one case per RT at its deepest tile class up to 3 that the width runs"""
    dpad = E.DIMS[dim]
    out = []
    for rt, nq, k in ((32, 65, 32), (64, 33, 33), (128, 32, 32)):
        rows = E.class_rows(rt)
        out.append((rows["t3"] if rows["t3"] <= E.rows_max(dpad) else rows["t2"], nq, k))
    return out


def _check(idx, ref, n, nq, k, alive, failures, tag, q=None):
    p = E.plan(n, nq, k, ref.dpad)
    s, r = idx.search(ref.q[:nq] if q is None else q, k)
    if q is not None:
        s, r = s.cpu().numpy(), r.cpu().numpy()
    g = idx.last_geometry()
    if (g["grid"], g["lds_bytes"], g["launches"]) != (p["grid"], p["lds_bytes"], 1):
        failures.append(f"{tag} n={n} nq={nq} k={k}: ran {g}, planned grid {p['grid']} with {p['lds_bytes']} LDS bytes")
    m = E.mismatch(s, r, *ref.topk(n, nq, k, alive))
    if m:
        failures.append(f"{tag} n={n} nq={nq} k={k} [{p['config']}]: {m}")
    return s, r


@pytest.mark.parametrize("dim", list(E.DIMS))
def test_removed_rows_are_absent_and_nothing_else_moves(rmu, dim):
    """holes: the first and the last row of a tile, a whole tile, a whole chunk and the best row of every query are deleted (at the
    geometry of each RT in turn); the reference drops the same rows."""
    steps = _steps(dim)
    ref = E.Reference(dim, "random", "ip", [E.Case(dim, "random", "ip", n, nq, k) for n, nq, k in steps])
    idx = rmu.FlatIndex(dim)
    idx.set_screening(False)
    alive = np.ones(ref.n_max, bool)
    failures, have = [], 0
    for n, nq, k in steps:
        idx.add(ref.x[have:n])
        have = n
        top1 = ref.topk(n, nq, 1, alive)[1][:, 0]
        dead = E.holes(E.plan(n, nq, k, ref.dpad), n, top1[top1 >= 0])
        dead = dead[alive[dead]]
        assert idx.remove_rows(dead) == dead.size
        alive[dead] = False
        for kk in (k, 1):
            _, r = _check(idx, ref, n, nq, kk, alive, failures, "holes")
            assert not np.isin(r, np.nonzero(~alive)[0]).any(), "a removed row was returned"
    _report(failures)


@pytest.mark.parametrize("dim", list(E.DIMS))
def test_host_and_device_queries_alone_and_in_a_batch_return_the_same_bits(rmu, dim):
    """The same queries alone and inside batches that change wq (1 -> 2 -> 4) and the number of query tiles, from host memory and from
    device memory (dim == dpad: the device form reads the caller's buffer in place), and an all-zero batch: rows 0..k-1, score bits 0."""
    import torch
    n = E.class_rows(32)["t3"]
    shapes = ((5, 32), (32, 32), (33, 32), (64, 33), (129, 32), (129, 112))
    ref = E.Reference(dim, "random", "ip", [E.Case(dim, "random", "ip", n, nq, k) for nq, k in shapes])
    idx = rmu.FlatIndex(dim)
    idx.set_screening(False)
    idx.add(ref.x[:n])
    failures, got = [], {}
    qd = torch.from_numpy(ref.q).cuda()
    for nq, k in shapes:
        got[(nq, k)] = _check(idx, ref, n, nq, k, None, failures, "host")
        sd, rd = _check(idx, ref, n, nq, k, None, failures, "device", q=qd[:nq])
        if E.mismatch(sd, rd, *got[(nq, k)]):
            failures.append(f"nq={nq} k={k}: device queries and host queries differ: " + E.mismatch(sd, rd, *got[(nq, k)]))
    for nq in (32, 33, 129):                                   # the first five queries: alone (w1), with 32 (w1), 33 (w2), 129 (w4, two tiles)
        m = E.mismatch(got[(nq, 32)][0][:5], got[(nq, 32)][1][:5], *got[(5, 32)])
        if m:
            failures.append(f"five queries alone and in a batch of {nq} differ: {m}")
    for nq, k in ((1, 1), (32, 32), (33, 33), (129, 112)):
        s, r = idx.search(np.zeros((nq, dim), np.float32), k)
        if not ((E.bits(s) == 0).all() and (r == np.arange(k)[None, :]).all()):
            failures.append(f"zero queries nq={nq} k={k}: rows {r[0][:8]}..., bits {E.bits(s)[0][:4]}")
    _report(failures)


def test_the_pin_tells_the_kernel_s_k_order_from_the_natural_one(rmu):
    """The same products summed in the order k = 0, 1, 2, ... are NOT what the kernel returns: for most (query, rank) pairs the
    natural-order score of the returned row has other bits, while the chain's has the returned bits (the test above)."""
    dim, n, nq, k = 384, E.class_rows(32)["t2"], 65, 32
    x, q = E.corpus("random", dim, n)
    idx = rmu.FlatIndex(dim)
    idx.set_screening(False)
    idx.add(x)
    s, r = idx.search(q[:nq], k)
    live = [i for i in range(nq) if i != E.ZERO_QUERY]
    nat = np.take_along_axis(E.cflat.chain_scores(q[:nq], x, dim, natural=True), r, axis=1)
    own = np.take_along_axis(E.chain(q[:nq], x, dim), r, axis=1)
    assert np.array_equal(E.bits(own), E.bits(s))
    assert (E.bits(nat) != E.bits(s))[live].mean() > 0.5


def test_the_last_row_count_before_the_deep_ladder_and_the_first_behind_it(rmu):
    """k = 33 over 262 143 rows is one launch of w2_k1 (promoted: 5 queries); one row more and the threshold ladder of the same kernel
    answers.  Both return the chain's bits."""
    dim, nq, k = 384, 5, 33
    ref = E.Reference(dim, "random", "ip", [E.Case(dim, "random", "ip", E.DEEP_N, nq, k)])
    idx = rmu.FlatIndex(dim)
    idx.set_screening(False)
    idx.add(ref.x[:E.DEEP_N - 1])
    failures = []
    _check(idx, ref, E.DEEP_N - 1, nq, k, None, failures, "below")
    idx.add(ref.x[E.DEEP_N - 1:])
    s, r = idx.search(ref.q[:nq], k)
    assert idx.last_geometry()["launches"] > 1, "the deep ladder did not take over at 262 144 rows"
    m = E.mismatch(s, r, *ref.topk(E.DEEP_N, nq, k))
    if m:
        failures.append(f"deep ladder at n={E.DEEP_N}: {m}")
    _report(failures)


@pytest.mark.parametrize("env", [{"RMU_NT": "0"}, {"RMU_NO_SHARED_THR": "1"}], ids=["no_nontemporal_stream", "no_shared_thresholds"])
def test_the_switched_forms_return_the_chain_bits(env):
    """The forms reached only through environment switches read at first use -- the plain (not non-temporal) w1_k0 and w2_k0, and
    share_thr = 0 -- in a fresh interpreter each, against the same expectations (tests/exact_variant_driver.py)."""
    here = os.path.dirname(os.path.abspath(__file__))
    out = subprocess.run([sys.executable, os.path.join(here, "exact_variant_driver.py")], env=dict(os.environ, RMU_TUNING="1", **env),
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    res = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    assert res["checked"] == len(E.variant_cases())
    if "RMU_NT" in env:
        assert {"w1_k0", "w2_k0"} <= set(res["configs"]) and not any(c.endswith("_nt") for c in res["configs"])
    _report(res["failures"])
