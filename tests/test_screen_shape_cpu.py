"""CPU: the 8-wave screening kernel's v_mfma_f32_16x16x32_f16 body (csrc/scan_screen.hip), checked as index arithmetic and as
numerics -- no GPU, no library call.

(a) the MFMA's own accumulator layout followed by the eight half-swaps (v_permlane32_swap) is the layout the candidate path was written
    for (lane (h, j) owns query j, rows 4h + 8i + c at element 4i + c) with lane bits 4 and 5 exchanged, for every (lane, register);
(b) the fragment reads -- lane l reads row 16 t + (l & 15), logical 16-byte unit 4 T' + (l >> 4) of a half-k chunk -- hit the bytes the DMA put
    there and are bank-conflict free under the ring's swizzle p ^ ((row >> 1) & 7), in the four lane groups ds_read_b128 is served in;
(c) twelve fp32 accumulations of 32 k each stay inside EPS(q) on the corpora of tests/test_screen_bound_cpu.py."""
import numpy as np
import pytest

from tests.test_screen_bound_cpu import corpora, eps, exact_scores_fp32, image

S_CKB = 384            # bytes per row per half-k chunk
LANES = np.arange(64)


# ---- (a) ownership ------------------------------------------------------------------------------------------------------------------------
def native_layout():
    """element e = 8 g + 4 t + c of lane l -> (query 16 g + (l & 15), row 16 t + 4 (l >> 4) + c): D of v_mfma_f32_16x16x32 with rows as A."""
    lay = np.empty((16, 64, 2), int)
    for g in range(2):
        for t in range(2):
            for c in range(4):
                lay[8 * g + 4 * t + c, :, 0] = 16 * g + (LANES & 15)
                lay[8 * g + 4 * t + c, :, 1] = 16 * t + 4 * (LANES >> 4) + c
    return lay


def permlane32_swap(vdst, src):
    """v_permlane32_swap_b32: lanes 32..63 of vdst change places with lanes 0..31 of src."""
    nd, ns = vdst.copy(), src.copy()
    nd[32:], ns[:32] = src[:32], vdst[32:]
    return nd, ns


def to_owner(nat):
    p = np.empty_like(nat)
    for t in range(2):
        for c in range(4):
            p[8 * t + c], p[8 * t + 4 + c] = permlane32_swap(nat[4 * t + c], nat[8 + 4 * t + c])
    return p


def test_half_swaps_restore_the_candidate_paths_ownership():
    got = to_owner(native_layout())
    for lane in range(64):
        b4, b5 = (lane >> 4) & 1, lane >> 5
        old = 32 * b4 + 16 * b5 + (lane & 15)                       # the lane of the 32x32x16 layout with bits 4 and 5 exchanged
        h, j = old >> 5, old & 31
        assert (h, j) == (b4, 16 * b5 + (lane & 15))                # what the kernel computes as h and j
        for r in range(16):
            i, c = r >> 2, r & 3
            assert tuple(got[r, lane]) == (j, 4 * h + 8 * i + c), (lane, r)
    # every (query, row) of the 32 x 32 tile exactly once, a query in exactly two lanes (lane ^ 16), a lane with ONE query
    cells = {tuple(v) for v in got.reshape(-1, 2)}
    assert len(cells) == 1024
    assert (got[:, :, 0] == got[0, :, 0]).all() and (got[0, LANES, 0] == got[0, LANES ^ 16, 0]).all()


def test_group_thresholds_from_one_half_swap():
    """thr_g0 / thr_g1 = permlane32_swap(thr, thr): the threshold of query (l & 15) and of query 16 + (l & 15) in every lane."""
    thr = 16 * (LANES >> 5) + (LANES & 15)                          # a lane's own query stands for its threshold
    g0, g1 = permlane32_swap(thr, thr)
    assert (g0 == (LANES & 15)).all() and (g1 == 16 + (LANES & 15)).all()


# ---- (b) fragment reads -------------------------------------------------------------------------------------------------------------------
def dma_phys_unit(row, unit):
    """where the DMA puts logical unit `unit` of row `row` of a chunk (dma_off: physical unit p holds logical unit p ^ ((row >> 1) & 7))"""
    return unit ^ ((row >> 1) & 7)


def frag_addr(lane, i):
    """byte address, inside a ring slot, of read i = 0..11 of a chunk: per-lane base (T' & 1) + immediates t * 6144 + (T' >> 1) * 128"""
    tp, t = i >> 1, i & 1
    n, g4 = lane & 15, lane >> 4
    base = n * S_CKB + (((4 * (tp & 1) + g4) ^ ((n >> 1) & 7)) * 16)
    return base + t * 16 * S_CKB + (tp >> 1) * 128


GROUPS = [[0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27], [4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31],
          [32, 33, 34, 35, 44, 45, 46, 47, 52, 53, 54, 55, 56, 57, 58, 59], [36, 37, 38, 39, 40, 41, 42, 43, 48, 49, 50, 51, 60, 61, 62, 63]]


def test_fragment_reads_address_the_dma_layout_and_cover_a_chunk():
    seen = set()
    for i in range(12):
        tp, t = i >> 1, i & 1
        for lane in range(64):
            row, unit = 16 * t + (lane & 15), 4 * tp + (lane >> 4)
            assert frag_addr(lane, i) == row * S_CKB + dma_phys_unit(row, unit) * 16, (i, lane)
            assert 0 <= frag_addr(lane, i) <= 32 * S_CKB - 16
            seen.add((row, unit))
    assert len(seen) == 32 * 24                                     # every 16-byte unit of the 32-row chunk, once


def test_fragment_reads_are_bank_conflict_free():
    assert sorted(sum(GROUPS, [])) == list(range(64))
    for slot in range(12):
        for i in range(12):
            for grp in GROUPS:
                banks = []
                for lane in grp:
                    a = slot * 32 * S_CKB + frag_addr(lane, i)
                    assert a % 16 == 0
                    banks += [(a // 4 + d) % 64 for d in range(4)]
                assert len(set(banks)) == 64, (slot, i, grp)


# ---- (c) numerics -------------------------------------------------------------------------------------------------------------------------
def screen_scores_32k(x, q):
    hx, hq = image(x).astype(np.float32), image(q).astype(np.float32)      # products of two fp16 values are exact in fp32
    acc = np.zeros((q.shape[0], x.shape[0]), np.float32)
    for k0 in range(0, x.shape[1], 32):                                   # one 16x16x32 MFMA step = 32 k, accumulated in fp32: 12 per score
        acc += (hq[:, k0:k0 + 32] @ hx[:, k0:k0 + 32].T).astype(np.float32)
    return acc * np.float32(1.0 / 4096.0)


@pytest.mark.parametrize("name,x,q", list(corpora()), ids=[c[0] for c in corpora()])
def test_twelve_step_accumulation_stays_within_eps(name, x, q):
    err = np.abs(screen_scores_32k(x, q).astype(np.float64) - exact_scores_fp32(x, q).astype(np.float64))
    bound = eps(x, q)[:, None]
    assert (err <= bound).all(), (name, float((err / bound).max()))
