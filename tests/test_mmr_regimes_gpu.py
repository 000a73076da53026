"""Both MMR selection kernels (k_mmr_lds and k_mmr behind launch_mmr, ragmeup_amd/csrc/rmu_api.hip) against an exact host reference, on
both sides of both dispatch thresholds.

tests/mmr_regimes.py holds the reference (exact products, math.fsum), the restated dispatch and the case table;
tests/test_mmr_regimes_cpu.py proves, without a GPU, that every greedy decision of every case is either a clear margin (>= 1e-10, some
thirty times what three summation orders can differ by) or an exact tie the kernels resolve on identical bits.  So every comparison here is
equality of the picked positions.
  * every case through rmu_index_mmr: the reference reads the rows the index STORES (rmu_index_get_rows: the rows given on an ip / l2
    index, the fp32-normalised rows on a cosine index), the output starts filled with a value no kernel writes and has a guard row behind it;
  * the device-pointer form (RMU_F_Q_DEVICE | RMU_F_OUT_DEVICE) on cases of both routes: the host form's answer, bit for bit;
  * rmu_index_search_mmr == rmu_index_search + rmu_index_mmr on the k_mmr route (dim 400), every metric, with a row_base;
  * the whole table and a search in a fresh process with RMU_TUNING=1 RMU_MMR_LDS=0 (the switch is read once): everything through k_mmr,
    still equal to the reference, and the digest of all answers equal to this process's -- "bit-identical picks" as a tested claim;
  * a removed row that a stale list still names is absent (the `*-removed-*` cases): before the fix both kernels took the NaN-poisoned row
    for a candidate of cosine 0 and returned it.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import mmr_regimes as M

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def rmu():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import ragmeup_amd
    from ragmeup_amd import _native
    _native.lib()                       # fails loudly if librmu.so is missing: there is no fallback
    return ragmeup_amd


@pytest.mark.parametrize("case", M.CASES, ids=lambda c: c.id)
def test_mmr_case(rmu, case):
    diff, _ = M.run_case(rmu, case)
    assert not diff, (case.id, M.route(case.dim, case.nq, M.lds_on_in_this_process()), diff)


_DEVICE_FORM = ["thr-dim384", "thr-dim385", "lds-fk64-dim384", "wave-nq5", "lds-k130-two-live", "wave-k130-two-live", "lds-list-all_absent",
                "wave-list-stale", "lds-metric-cosine", "wave-metric-l2", "lds-removed-ip", "wave-removed-ip"]


@pytest.mark.parametrize("case", [M.CASE_BY_ID[i] for i in _DEVICE_FORM], ids=lambda c: c.id)
def test_mmr_with_device_pointers_equals_the_host_form(rmu, case):
    """q, the lists and out_pos as device addresses of torch tensors, through ctypes (FlatIndex.mmr always passes flags = 0)."""
    diff_d, got_d = M.run_case(rmu, case, device=True)
    diff_h, got_h = M.run_case(rmu, case)
    assert not diff_d and not diff_h, (case.id, diff_d, diff_h)
    assert got_d.dtype == got_h.dtype == np.int32 and np.array_equal(got_d, got_h)


def test_device_form_covers_both_routes():
    assert {M.CASE_BY_ID[i].route for i in _DEVICE_FORM} == {"lds", "wave"}


@pytest.mark.parametrize("nq", [1, 5])
@pytest.mark.parametrize("metric", ["ip", "cosine", "l2"])
def test_search_mmr_equals_search_then_mmr_on_the_wave_route(rmu, metric, nq):
    """dim 400 takes k_mmr (tests/test_search_gpu.py covers the one call at 384 only): rows in pick order with the row_base, their search
    scores, and the picks equal to the reference on the stored rows."""
    from ragmeup_amd import _native as N
    dim, n, fetch_k, k, lam, base = 400, 300, 20, 10, 0.35, 5000
    assert M.route(dim, nq) == "wave"
    rng = np.random.default_rng(400 + nq)
    x = rng.standard_normal((n, dim)).astype(np.float32)
    q = (x[:nq] + 0.6 * rng.standard_normal((nq, dim))).astype(np.float32)
    idx = rmu.FlatIndex(dim, metric={"ip": N.METRIC_IP, "cosine": N.METRIC_COSINE, "l2": N.METRIC_L2SQ}[metric], capacity_hint=n)
    try:
        idx.add(x)
        s, r = idx.search(q, fetch_k)
        pos = idx.mmr(q, r, k, lam)
        rows, sc = idx.search_mmr(q, fetch_k, k, lam, row_base=base)
        stored = idx.get_rows(np.arange(n, dtype=np.int64))
    finally:
        idx.close()
    assert (r >= 0).all() and (pos >= 0).all()
    assert np.array_equal(rows, np.take_along_axis(r, pos.astype(np.int64), axis=1) + base)
    assert np.array_equal(sc.view(np.uint32), np.take_along_axis(s, pos.astype(np.int64), axis=1).view(np.uint32))
    for i in range(nq):
        picks, margins, ties = M.ref_mmr(q[i], stored[r[i]], [True] * fetch_k, k, lam)
        assert min(margins) >= M.MARGIN_MIN and not any(ties)
        assert pos[i].tolist() == picks


def test_both_kernels_return_the_same_picks():
    """The case table and one search + selection at dim 384 here (k_mmr_lds wherever launch_mmr allows it) and in a fresh process with
    RMU_TUNING=1 RMU_MMR_LDS=0 (tests/mmr_variant_driver.py: k_mmr everywhere).  Every case must equal the reference in both, and the
    digests of all answers must be equal: the form of the selection does not change a pick."""
    import ragmeup_amd
    assert M.lds_on_in_this_process(), "run the suite without RMU_MMR_LDS=0: this test needs the default form in its own process"
    here = M.run_all(ragmeup_amd)
    assert not here["failed"] and here["search_ok"] and here["routes"] == ["lds", "wave"] and here["cases"] == len(M.CASES)
    env = {k: v for k, v in os.environ.items() if k != "RMU_MMR_LDS"}
    env.update(RMU_TUNING="1", RMU_MMR_LDS="0")
    out = subprocess.run([sys.executable, os.path.join(HERE, "mmr_variant_driver.py")], env=env, capture_output=True, text=True,
                         timeout=120)       # measured: 2.6 s for this whole test, the interpreter's start (import torch) included
    assert out.returncode == 0, out.stderr[-2000:]
    there = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    assert there["lds_on"] is False and there["cases"] == len(M.CASES)
    assert not there["failed"], there["failed"]
    assert there["routes"] == ["wave"] and there["search_ok"]
    assert there["digest"] == here["digest"]
