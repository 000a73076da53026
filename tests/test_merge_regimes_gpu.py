"""Every kernel of ragmeup_amd/csrc/topk_merge.hip against an exact host reference, in every dispatch regime.

tests/merge_regimes.py holds the references, the restated dispatch and the case table (tests/test_merge_regimes_cpu.py checks, without
a GPU, that the table reaches every route and threshold from both sides).  The launchers are called directly -- librmu.so exports them
under their C++ names -- with device pointers of torch tensors; the merge is integer code over u64 keys, so every comparison is equality,
scores as bit patterns, whole output arrays with the regions nobody may write.
  * key merges (rmu_merge_to_keys_launch, rmu_merge_final_launch): merge_select_kernel in its four instantiations, its tau step at
    parts around k, its candidate array at exactly CAPM keys and one more (the fallback), unsorted = 1 on lists that really are
    unsorted, merge_wg_kernel beyond 1024 parts, and every MergeOut field (row_base, scatter, l2_out, cond, seed_thr);
  * the same cases with RMU_TUNING=1 RMU_MERGE_SELECT=0 in a fresh process (the switch is read once): merge_wg_kernel at every wpq and in
    both NPL, and a search end to end whose answers must not change by a bit with the form of the merge;
  * merge_lists_kernel (rmu_merge_lists_launch, rmu_topk_merge): strides, the all-gather's packed buffer, both directions, ties, NaN,
    holes, +-inf, +-0;
  * the refusals.

Zeros in the list merge: the kernel builds its keys from s + 0.0f (or -s + 0.0f), so -0 and +0 are ONE score, ordered by candidate index,
and come out as +0 in both directions.  (The distance direction used to return -0.0 for an exact hit -- the negation of the key's +0 --
while the single-index L2 search returns +0 = max(|q|^2 - s, 0); the kernel now writes 0 - s.)
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests import merge_regimes as M

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


@pytest.fixture(scope="module")
def lib(rmu):
    from ragmeup_amd import _native
    return _native.lib()


@pytest.fixture(scope="module")
def fns(lib):
    return M.launchers(lib)


@pytest.mark.parametrize("case", M.CASES, ids=lambda c: c.id)
def test_key_merge_case(fns, case):
    diff = M.run_key_case(fns, case)
    assert not diff, (case.id, case.route, diff)


def _run_lists(fns, case, s, rows):
    import torch
    dev = torch.device("cuda", 0)
    bufs, off_s, off_r, ss, sr = M.lay_out(case, s, rows)
    dbufs = [torch.from_numpy(b).to(dev) for b in bufs]
    out_s = torch.from_numpy(np.full((case.nq, case.k), M.FILL_BITS, np.uint32).view(np.int32)).to(dev)
    out_r = torch.full((case.nq, case.k), int(M.FILL_ROW), dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    rc = fns["lists"](dbufs[0].data_ptr() + off_s, dbufs[-1].data_ptr() + off_r, case.parts, ss, sr, case.nq, case.k, int(case.smaller_better),
                      out_s.data_ptr(), out_r.data_ptr(), None)
    torch.cuda.synchronize()
    assert rc == 0
    return out_s.cpu().numpy().view(np.float32), out_r.cpu().numpy()


def _check_lists(got_s, got_r, s, rows, k, smaller_better):
    want_s, want_r, _ = M.ref_lists(s, rows, k, smaller_better)
    assert np.array_equal(got_r, want_r)                                     # rows: exact, the tie rule (lower part, earlier position) included
    assert not np.isnan(got_s).any() and np.array_equal(got_s, want_s)      # == : a zero equals a zero
    nz = want_s != 0
    assert np.array_equal(got_s.view(np.uint32)[nz], want_s.view(np.uint32)[nz])
    assert (got_s.view(np.uint32)[~nz] == 0).all()                           # ... and a zero comes out as +0, similarity or distance


@pytest.mark.parametrize("case", M.LIST_CASES, ids=lambda c: c.id)
def test_list_merge_case(fns, case):
    s, rows = M.build_list_case(case)
    got_s, got_r = _run_lists(fns, case, s, rows)
    _check_lists(got_s, got_r, s, rows, case.k, case.smaller_better)


def test_list_merge_returns_plus_zero_for_an_exact_hit_in_both_directions(fns):
    """Two parts, one query: -0 in part 0 and +0 in part 1 are the same score, part 0 wins the tie, and the result is +0 either way."""
    case = M.ListCase("zeros", 2, 1, 3, True, "packed")
    s = np.array([[[1.0, -0.0, 2.0]], [[0.0, 0.5, -0.0]]], np.float32)
    rows = np.array([[[10, 11, 12]], [[20, 21, 22]]], np.int64)
    for sb, want_r in ((True, [11, 20, 22]), (False, [12, 10, 21])):
        c = M.ListCase("zeros", 2, 1, 3, sb, "packed")
        got_s, got_r = _run_lists(fns, c, s, rows)
        assert got_r[0].tolist() == want_r
        _check_lists(got_s, got_r, s, rows, 3, sb)
    got_s, _ = _run_lists(fns, case, s, rows)
    assert got_s.view(np.uint32)[0].tolist() == [0, 0, 0]


@pytest.mark.parametrize("in_dev,out_dev", [(False, False), (True, True), (False, True), (True, False)], ids=["host-host", "dev-dev", "host-dev", "dev-host"])
@pytest.mark.parametrize("k,parts,nq,sb", [(10, 8, 7, False), (65, 13, 4, True), (128, 2, 1, False)])
def test_topk_merge_entry_point(lib, in_dev, out_dev, k, parts, nq, sb):
    """rmu_topk_merge with every combination of host and device lists and results (the packed layout, the library's own stream)."""
    import torch
    from ragmeup_amd import _native as N
    case = M.ListCase(f"abi-k{k}-p{parts}-nq{nq}", parts, nq, k, sb, "packed")
    s, rows = M.build_list_case(case)
    dev = torch.device("cuda", 0)
    flags = (N.F_Q_DEVICE if in_dev else 0) | (N.F_OUT_DEVICE if out_dev else 0) | (N.F_SMALLER_BETTER if sb else 0)
    s_d, r_d = torch.from_numpy(s).to(dev), torch.from_numpy(rows).to(dev)
    o_s = np.full((nq, k), M.FILL_BITS, np.uint32).view(np.float32)
    o_r = np.full((nq, k), M.FILL_ROW, np.int64)
    os_d, or_d = torch.from_numpy(o_s).to(dev), torch.from_numpy(o_r).to(dev)
    torch.cuda.synchronize()
    rc = lib.rmu_topk_merge(s_d.data_ptr() if in_dev else s.ctypes.data, r_d.data_ptr() if in_dev else rows.ctypes.data, parts, nq, k, flags,
                               os_d.data_ptr() if out_dev else o_s.ctypes.data, or_d.data_ptr() if out_dev else o_r.ctypes.data, 0)
    torch.cuda.synchronize()
    assert rc == 0
    got_s, got_r = (os_d.cpu().numpy(), or_d.cpu().numpy()) if out_dev else (o_s, o_r)
    _check_lists(got_s, got_r, s, rows, k, sb)


def test_refusals(fns):
    """k = 0, k = 129, parts = 0, nq = 0 (and negatives) return RMU_E_INVALID from every launcher, parts * k = 2^32 from the list merge,
    and nothing is launched: the outputs keep their fill."""
    import torch
    dev = torch.device("cuda", 0)
    lists = torch.zeros(4 * 3 * 129, dtype=torch.int64, device=dev)
    sc = torch.zeros(4 * 3 * 129, dtype=torch.float32, device=dev)
    keys = torch.full((3 * 129,), -3, dtype=torch.int64, device=dev)
    seed = torch.full((3,), 5, dtype=torch.int32, device=dev)
    out_s = torch.full((3 * 129,), 7.0, dtype=torch.float32, device=dev)
    out_r = torch.full((3 * 129,), int(M.FILL_ROW), dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    for k, parts, nq in M.REFUSED:
        assert M.route(parts, nq, k) == ("invalid",)
        assert fns["to_keys"](lists.data_ptr(), parts, nq, k, keys.data_ptr(), seed.data_ptr(), None, 0) == M.E_INVALID, (k, parts, nq)
        assert fns["final"](lists.data_ptr(), parts, nq, k, 0, 0, None, out_s.data_ptr(), out_r.data_ptr(), None, None, None) == M.E_INVALID, (k, parts, nq)
        assert fns["lists"](sc.data_ptr(), lists.data_ptr(), parts, nq * k, nq * k, nq, k, 0, out_s.data_ptr(), out_r.data_ptr(), None) == M.E_INVALID, (k, parts, nq)
    for k, parts, nq in M.REFUSED_LISTS_ONLY:
        assert parts * k >= 2 ** 32 and (parts - 1) * k < 2 ** 32
        assert fns["lists"](sc.data_ptr(), lists.data_ptr(), parts, nq * k, nq * k, nq, k, 0, out_s.data_ptr(), out_r.data_ptr(), None) == M.E_INVALID
    torch.cuda.synchronize()
    assert (keys == -3).all() and (seed == 5).all() and (out_s == 7.0).all() and (out_r == int(M.FILL_ROW)).all()


def test_both_forms_of_the_merge_return_the_same_answers():
    """The case table and one search end to end (96 queries through the screening ladder at k = 10, 7 queries through the exact scans at
    k = 100, 300 000 rows) in two fresh processes: the default, and RMU_TUNING=1 RMU_MERGE_SELECT=0, where every merge is
    merge_wg_kernel's -- wpq 1, 2, 4, 8 and 16, NPL 1 and 2.  Every case must equal the reference in both, and the searches' digests
    must be equal: the form of the merge does not change a bit of an answer."""
    env = {k: v for k, v in os.environ.items() if k not in ("RMU_TUNING", "RMU_MERGE_SELECT")}
    res = {}
    for name, extra in (("select", {}), ("wg", {"RMU_TUNING": "1", "RMU_MERGE_SELECT": "0"})):
        out = subprocess.run([sys.executable, os.path.join(HERE, "merge_variant_driver.py")], env=dict(env, **extra), capture_output=True, text=True,
                             timeout=300)           # ~190 small merges, a 300 000-row index and two searches: well under a minute
        assert out.returncode == 0, (name, out.stderr[-2000:])
        r = res[name] = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
        assert r["select"] == (name == "select") and r["cases"] == len(M.CASES)
        assert not r["failed"], (name, r["failed"])
        assert all(v["ok"] for v in r["search"].values()), (name, r["search"])
    assert {tuple(v) for v in res["wg"]["routes"]} == {("wg", npl, w) for npl in (1, 2) for w in (1, 2, 4, 8, 16)}
    assert {tuple(v)[0] for v in res["select"]["routes"]} == {"select", "wg"}
    assert res["select"]["digest"] == res["wg"]["digest"] and res["select"]["search"] == res["wg"]["search"]
