"""The gathered exact scan (`scan_subset_kernel`, `scan_groups_kernel`) held to the fmaf chain of the exact scan, bit for bit, in every
geometry.

tests/subset_regimes.py restates rmu_subset_plan and rmu_groups_plan and lists the cases: every (padded width x S_w1_k0 / S_w4_k0 /
S_w4_k1) with 1, 2, 3 (and, at 32 rows per tile, 4) tiles per workgroup, both block-map branches, one and two query tiles, every nq / k
boundary of the planner from both sides, rising / falling corpora, COSINE and L2 indexes, and grouped calls with 3 tiles per workgroup
in either class, with group boundaries inside a query fragment, null descriptors and a Pcap-bound group.  The lists are NOT contiguous:
position and row id differ everywhere, they hold some -- never the lowest id, never all -- of every flood cluster, and more than a full
slot of bit-identical best rows across a chunk boundary of the plan.  Here every case must
  * have run the planned geometry: FlatIndex.last_geometry() == the planned grid and LDS bytes, in one launch (grouped: one launch per
    class present, grid and LDS bytes of the last class);
  * return the reference's score BITS and row ids (exact_regimes' chain, ranked over the rows the list names).  There is no tolerance and
    no tie rule in this file: equal scores are ordered by row id, which is the order of the list.
The queries of every case are a prefix of ONE batch per family, so a query's bits are also compared across the batch sizes it travels with.
"""
from types import SimpleNamespace

import numpy as np
import pytest

from tests import exact_regimes as E
from tests import subset_regimes as S

pytestmark = pytest.mark.gpu

FAMILIES = S.families()
DIM = 384                                              # the width of everything below the grid
# one (configuration, list length, nq, k) per geometry, 3 tiles per workgroup each
GEOMETRIES = (("S_w1_k0", S.class_lengths(128)["t3"], 32, 32), ("S_w4_k0", S.class_lengths(32)["t3"], 128, 32),
              ("S_w4_k1", S.class_lengths(32)["t3"], 32, 33))


@pytest.fixture(scope="module")
def rmu():
    import torch
    assert torch.cuda.is_available(), "GPU tests need an MI355X"
    import ragmeup_amd
    from ragmeup_amd import _native
    _native.lib()
    return ragmeup_amd


@pytest.fixture(scope="module")
def ref():
    """the chain scores of the `random` corpus of DIM, every row of its index, for both query buckets: shared, never changed"""
    n = S.N_ROWS[E.DIMS[DIM]]
    return S.Reference(DIM, "random", "ip", [SimpleNamespace(nq=32, n=n), SimpleNamespace(nq=S.NQ_MAX, n=n)])


@pytest.fixture(scope="module")
def index(rmu, ref):
    """an index of those rows that no test changes"""
    idx = rmu.FlatIndex(DIM)
    idx.add(ref.x[:ref.n_max])
    yield idx
    idx.close()


def _report(failures):
    assert not failures, f"{len(failures)} mismatches:\n" + "\n".join(failures[:12])


def _list(config, length):
    p = S.subset_plan(length, 32 if config == "S_w1_k0" else 128, 32 if config != "S_w4_k1" else 33, E.DIMS[DIM])
    return S.make_list(length, S.span_of(length, E.DIMS[DIM]), p["RT"] * p["tiles_per_chunk"])


def _np(t):
    return t.cpu().numpy() if hasattr(t, "cpu") else t


def _geometry(idx, p, failures, what):
    g = S.geometry_mismatch(idx.last_geometry(), p["grid"], p["lds_bytes"], 1)
    if g:
        failures.append(f"{what}: {g}")


@pytest.mark.parametrize("family", list(FAMILIES), ids=["-".join(map(str, f)) for f in FAMILIES])
def test_every_case_runs_its_geometry_and_returns_the_chain_bits(rmu, family):
    """IP: scores and rows of the list's rows ranked on the chain.  COSINE and L2: the chain over the restated images and, for L2, the
    restated merge step max(|q|^2 - s, 0)."""
    failures, checked = S.run_family(rmu.FlatIndex, family, FAMILIES[family])
    assert checked == len(FAMILIES[family])
    _report(failures)


def test_absent_ids_in_a_device_list_are_skipped_and_nothing_else_moves(index, ref):
    """Device lists are not validated.  Ids >= n, >= 2^31, >= 2^32 (whose low 32 bits name a row) and negative ones stand at the first
    and the last position of a list tile, fill a whole tile, fill a whole chunk and end the list: the answer is that of the list
    without them."""
    import torch
    n = len(index)
    qd = torch.from_numpy(ref.q).cuda()
    failures = []
    for config, length, nq, k in GEOMETRIES:
        rows = _list(config, length)
        p = S.subset_plan(length, nq, k, ref.dpad)
        assert p["config"] == config and p["tiles_per_chunk"] == 3
        rt, chunk = p["RT"], p["RT"] * p["tiles_per_chunk"]
        where = np.unique(np.concatenate([[5 * rt, 6 * rt - 1], 9 * rt + np.arange(rt), 3 * chunk + np.arange(chunk), length - 7 + np.arange(7)]))
        bad = np.array([(n + 5 + i, (1 << 31) + i, (1 << 32) + i, -1 - i)[i % 4] for i in range(where.size)], np.int64)
        holed = rows.copy()
        holed[where] = bad
        s, r = index.search(qd[:nq], k, rows=torch.from_numpy(holed).cuda())
        _geometry(index, p, failures, f"{config} absent ids")
        m = E.mismatch(_np(s), _np(r), *ref.expected(np.delete(rows, where), nq, k))
        if m:
            failures.append(f"{config} L={length} nq={nq} k={k} with {where.size} absent ids: {m}")
    _report(failures)


def test_removed_rows_are_absent_and_nothing_else_moves(rmu, ref):
    """exact_regimes.holes over the POSITIONS of each geometry's list: the rows at the first and the last position of a list tile, a
    whole list tile, a whole chunk and the best row of every query are removed from the index; the reference drops the same rows."""
    idx = rmu.FlatIndex(DIM)
    idx.add(ref.x[:ref.n_max])
    removed = np.zeros(ref.n_max, bool)
    failures = []
    for config, length, nq, k in GEOMETRIES:
        rows = _list(config, length)
        p = S.subset_plan(length, nq, k, ref.dpad)
        top1 = ref.expected(rows, nq, 1, alive=~removed[rows])[1][:, 0]
        dead = np.union1d(rows[E.holes(p, length, [])], top1[top1 >= 0])
        dead = dead[~removed[dead]]
        assert idx.remove_rows(dead) == dead.size
        removed[dead] = True
        for kk in (k, 1):
            s, r = idx.search(ref.q[:nq], kk, rows=rows)
            _geometry(idx, S.subset_plan(length, nq, kk, ref.dpad), failures, f"{config} holes")
            assert not removed[r[r >= 0]].any(), "a removed row was returned"
            m = E.mismatch(s, r, *ref.expected(rows, nq, kk, alive=~removed[rows]))
            if m:
                failures.append(f"{config} L={length} nq={nq} k={kk} with {int(removed.sum())} rows removed: {m}")
    idx.close()
    _report(failures)


@pytest.mark.parametrize("metric", ["ip", "l2"])
def test_fewer_live_rows_than_k_pads_the_answer(rmu, metric):
    """An empty list, lists shorter than k and all-absent device lists: the tail is (-inf, -1), or (+inf, -1) on an L2 index."""
    import torch
    dim = 100
    n = E.FLOOD_END
    ref = S.Reference(dim, "scaled", metric, [SimpleNamespace(nq=S.NQ_MAX, n=n), SimpleNamespace(nq=32, n=n)])
    idx = rmu.FlatIndex(dim, metric=E._METRIC[metric])
    idx.add(ref.x[:n])
    qd = torch.from_numpy(ref.q).cuda()
    pad = np.float32(np.inf if metric == "l2" else -np.inf)
    failures = []
    for nq, k in ((5, 32), (40, 32), (5, 112), (129, 33)):
        for length in (0, 1, k - 1, 20):
            rows = S.make_list(length, n, 32) if length else np.empty(0, np.int64)
            s, r = idx.search(ref.q[:nq], k, rows=rows)
            if length == 0:
                assert idx.last_geometry()["launches"] == 0, "an empty list launched a scan"
            else:
                _geometry(idx, S.subset_plan(length, nq, k, ref.dpad), failures, f"L={length} nq={nq} k={k}")
            live = min(length, k)
            assert (r[:, live:] == -1).all() and (s[:, live:] == pad).all() and (r[:, :live] >= 0).all()
            m = E.mismatch(s, r, *ref.expected(rows, nq, k))
            if m:
                failures.append(f"L={length} nq={nq} k={k}: {m}")
        for length in (50, 300):                           # every id absent: the scan runs and nothing passes
            rows = np.array([(n + i, (1 << 32) + i, -1 - i)[i % 3] for i in range(length)], np.int64)
            s, r = idx.search(qd[:nq], k, rows=torch.from_numpy(rows).cuda())
            _geometry(idx, S.subset_plan(length, nq, k, ref.dpad), failures, f"all-absent L={length} nq={nq} k={k}")
            if not ((_np(r) == -1).all() and (_np(s) == pad).all()):
                failures.append(f"all-absent list of {length}, nq={nq} k={k}: something was returned")
    idx.close()
    _report(failures)


def test_every_form_of_the_call_returns_the_bits_of_the_plain_one(index, ref):
    """Host and device queries and lists, row_base, a caller stream with out=: one geometry each, against the plain host call, which
    itself returns the reference."""
    import torch
    qd = torch.from_numpy(ref.q).cuda()
    base = 1_000_000
    failures = []
    for config, length, nq, k in GEOMETRIES:
        rows = _list(config, length)
        p = S.subset_plan(length, nq, k, ref.dpad)
        rd = torch.from_numpy(np.array(rows)).cuda()
        plain = index.search(ref.q[:nq], k, rows=rows)
        m = E.mismatch(*plain, *ref.expected(rows, nq, k))
        if m:
            failures.append(f"{config} plain: {m}")
        shifted = (plain[0], np.where(plain[1] >= 0, plain[1] + base, -1))
        st = torch.cuda.Stream()
        out = (torch.empty((nq, k), dtype=torch.float32, device="cuda"), torch.empty((nq, k), dtype=torch.int64, device="cuda"))
        forms = {"device queries, host list": lambda: (index.search(qd[:nq], k, rows=rows), plain),
                 "device queries, device list": lambda: (index.search(qd[:nq], k, rows=rd), plain),
                 "host, row_base": lambda: (index.search(ref.q[:nq], k, row_base=base, rows=rows), shifted),
                 "device, row_base": lambda: (index.search(qd[:nq], k, row_base=base, rows=rd), shifted)}
        for name, form in forms.items():
            got, want = form()
            _geometry(index, p, failures, f"{config} {name}")
            m = E.mismatch(_np(got[0]), _np(got[1]), *want)
            if m:
                failures.append(f"{config} {name}: {m}")
        torch.cuda.synchronize()
        with torch.cuda.stream(st):
            got = index.search(qd[:nq], k, row_base=base, stream=st.cuda_stream, out=out, rows=rd)
        st.synchronize()
        assert got[0] is out[0] and got[1] is out[1]
        _geometry(index, p, failures, f"{config} caller stream")
        m = E.mismatch(_np(out[0]), _np(out[1]), *shifted)
        if m:
            failures.append(f"{config} caller stream, out=, row_base: {m}")
    _report(failures)


@pytest.mark.parametrize("name", [c.name for c in S.group_calls(DIM)])
def test_a_grouped_call_runs_its_tables_and_every_query_returns_the_chain_bits_of_its_list(index, ref, name):
    """rmu_index_search_groups: the planned launches (one per class present; grid and LDS bytes of the last) and, per query, the chain
    reference over ITS list -- not the per-list call, which is the same tile loop.  The mixed call also from device lists."""
    call = {c.name: c for c in S.group_calls(DIM)}[name]
    failures = S.run_group_call(index, ref, call)
    if name == "mixed":
        failures += [f"device lists: {f}" for f in S.run_group_call(index, ref, call, device_lists=True)]
    _report(failures)


def test_the_pin_tells_the_kernel_s_k_order_from_the_natural_one(index, ref):
    """A 2-tile S_w1_k0 case: the same products summed in the order k = 0, 1, 2, ... do NOT have the returned bits for most (query, rank)
    pairs, while the chain's has them.  The queries are S.PIN_QUERIES, none aimed at a flood cluster: a cluster's query returns 32 copies of
    ONE row, which is one pair counted 32 times (all of them differ or none does)."""
    length, k = S.class_lengths(128)["t2"], 32
    qi = np.arange(*S.PIN_QUERIES)
    rows = _list("S_w1_k0", length)
    p = S.subset_plan(length, qi.size, k, ref.dpad)
    assert p["config"] == "S_w1_k0" and p["tiles_per_chunk"] == 2 and E.ZERO_QUERY not in qi
    s, r = index.search(ref.q[qi], k, rows=rows)
    failures = []
    _geometry(index, p, failures, "pin")
    _report(failures)
    x = ref.x[:int(rows[-1]) + 1]
    nat = np.take_along_axis(E.cflat.chain_scores(ref.q[qi], x, DIM, natural=True), r, axis=1)
    own = np.take_along_axis(E.chain(ref.q[qi], x, DIM), r, axis=1)
    assert np.array_equal(E.bits(own), E.bits(s))
    assert (E.bits(nat) != E.bits(s)).mean() > 0.5
