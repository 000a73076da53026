"""GPU: rmu_rrf_fuse (rrf_fuse.hip) alone, through host and through device pointers, against the pure-Python fusion of tests/rrf_ref.py:
keys and representatives identical, scores equal as bits."""
import ctypes

import numpy as np
import pytest

from tests.rrf_ref import fuse_arrays, random_case

pytestmark = pytest.mark.gpu


def _weights(kind, lists, rng):
    if kind == "equal":
        return [1.0 / lists] * lists
    if kind == "random":
        return rng.uniform(0.0, 1.0, lists).tolist()
    return [1.0] + [0.0] * (lists - 1)


def _fuse(keys, weights, c, k_out, device=False):
    from ragmeup_amd import _native as N
    lib = N.lib()
    lists, nq, depth = keys.shape
    w = (ctypes.c_double * lists)(*weights)
    if not device:
        keys = np.ascontiguousarray(keys)
        s, k, r = np.empty((nq, k_out), np.float64), np.empty((nq, k_out), np.int64), np.empty((nq, k_out), np.int32)
        N.check(lib.rmu_rrf_fuse(keys.ctypes.data, lists, nq, depth, w, c, k_out, 0, s.ctypes.data, k.ctypes.data, r.ctypes.data, 0), "rmu_rrf_fuse")
        return s, k, r
    import torch
    dk = torch.from_numpy(np.ascontiguousarray(keys)).cuda()
    s = torch.empty((nq, k_out), dtype=torch.float64, device="cuda")
    k = torch.empty((nq, k_out), dtype=torch.int64, device="cuda")
    r = torch.empty((nq, k_out), dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    N.check(lib.rmu_rrf_fuse(dk.data_ptr(), lists, nq, depth, w, c, k_out, N.F_Q_DEVICE | N.F_OUT_DEVICE, s.data_ptr(), k.data_ptr(), r.data_ptr(),
                             st.cuda_stream), "rmu_rrf_fuse")
    st.synchronize()
    return s.cpu().numpy(), k.cpu().numpy(), r.cpu().numpy()


def _same(got, want, what):
    s, k, r = got
    ws, wk, wr = want
    assert np.array_equal(k, wk), what
    assert np.array_equal(r, wr), what
    assert np.array_equal(s.view(np.int64), ws.view(np.int64)), what


@pytest.mark.parametrize("depth", [1, 4, 20, 64, 112])
@pytest.mark.parametrize("lists", [1, 2, 3, 4])
def test_random_grid_matches_python_bit_for_bit(lists, depth):
    rng = np.random.default_rng(1000 * lists + depth)
    k_out = lists * depth
    ties = 0
    for nq in (1, 3, 65, 1000):
        keys = random_case(rng, lists, nq, depth)
        for kind in ("equal", "random", "first_only"):
            w = _weights(kind, lists, rng)
            for c in (60, 0, 1):
                want = fuse_arrays(keys, w, c, k_out)
                fin = np.isfinite(want[0])
                ties += int(((want[0][:, 1:] == want[0][:, :-1]) & fin[:, 1:]).sum())
                _same(_fuse(keys, w, c, k_out), want, (nq, kind, c, "host"))
                if c == 60 or nq == 65:
                    _same(_fuse(keys, w, c, k_out, device=True), want, (nq, kind, c, "device"))
    if lists > 1:
        assert ties > 0            # the tie rule was exercised


def test_disjoint_lists_with_equal_weights_tie_pairwise_and_list_0_comes_first():
    depth, nq = 20, 3
    keys = np.stack([np.tile(np.arange(depth), (nq, 1)), np.tile(np.arange(depth) + 1000, (nq, 1))]).astype(np.int64)
    s, k, r = _fuse(keys, [0.5, 0.5], 60, 2 * depth)
    for rank in range(depth):
        assert np.all(k[:, 2 * rank] == rank) and np.all(k[:, 2 * rank + 1] == 1000 + rank)
        assert np.all(r[:, 2 * rank] == rank) and np.all(r[:, 2 * rank + 1] == depth + rank)
        assert np.all(s[:, 2 * rank] == s[:, 2 * rank + 1]) and np.all(s[:, 2 * rank] == 0.5 / (rank + 1 + 60))
    _same((s, k, r), fuse_arrays(keys, [0.5, 0.5], 60, 2 * depth), "disjoint")


def test_k_out_truncates_and_pads():
    rng = np.random.default_rng(5)
    keys = random_case(rng, 3, 7, 20)
    keys[:, 0] = np.arange(60).reshape(3, 20)            # query 0: 60 distinct keys
    keys[:, 1] = -1
    keys[:, 1, :5] = [[4, 4, 9, 4, 9]] * 3               # query 1: 2 distinct keys
    w = [0.2, 0.5, 0.3]
    full = fuse_arrays(keys, w, 60, 60)
    for device in (False, True):
        for k_out in (1, 5, 59):                         # below the distinct count of query 0: the head of the full list
            got = _fuse(keys, w, 60, k_out, device)
            _same(got, tuple(a[:, :k_out] for a in full), k_out)
        s, k, r = _fuse(keys, w, 60, 60, device)
        _same((s, k, r), full, 60)
        assert np.all(k[1, 2:] == -1) and np.all(r[1, 2:] == -1) and np.all(np.isneginf(s[1, 2:])) and np.all(k[1, :2] >= 0)


def test_absent_slots_in_the_middle_of_a_list_consume_no_rank():
    a = np.array([[[7, -1, -1, 8, -1, 9]], [[-1, 9, -1, -1, 7, 30]]], np.int64)
    b = np.array([[[7, 8, 9, -1, -1, -1]], [[9, 7, 30, -1, -1, -1]]], np.int64)
    w = [0.6, 0.4]
    sa, ka, ra = _fuse(a, w, 60, 12)
    sb, kb, rb = _fuse(b, w, 60, 12)
    assert np.array_equal(ka, kb) and np.array_equal(sa.view(np.int64), sb.view(np.int64))
    assert ka[0, :4].tolist() == [7, 9, 8, 30] and ra[0, :4].tolist() == [0, 5, 3, 11] and rb[0, :4].tolist() == [0, 2, 1, 8]
    assert sa[0, 0] == 0.0 + 0.6 / 61 + 0.4 / 62 and sa[0, 1] == 0.0 + 0.6 / 63 + 0.4 / 61
    _same((sa, ka, ra), fuse_arrays(a, w, 60, 12), "middle")
