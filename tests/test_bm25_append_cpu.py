"""CPU: the interface of the append path of the BM25 index (include/rmu.h: RMU_BM25_OPT_REPACK_ON_ADD, RMU_BM25_STAT_IMAGE_*) -- the switch and
the three image counters are host-only -- and the splice kernel's code object."""
import ctypes
import os

import pytest

from tests.test_bm25_cpu import _tricky_corpus


def test_binding_lists_the_new_constants(librmu):
    from ragmeup_amd import _native
    assert _native.BM25_OPT_REPACK_ON_ADD == 8
    assert (_native.BM25_STAT_IMAGE_PACKS, _native.BM25_STAT_IMAGE_SPLICES, _native.BM25_STAT_IMAGE_UPLOAD_BYTES) == (16, 17, 18)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "rmu.h"), encoding="utf-8").read()
    for name in ("OPT_REPACK_ON_ADD", "STAT_IMAGE_PACKS", "STAT_IMAGE_SPLICES", "STAT_IMAGE_UPLOAD_BYTES"):
        assert f"#define RMU_BM25_{name} {getattr(_native, 'BM25_' + name)}" in header, name


def test_the_switch_takes_0_or_1_and_the_counters_read_0_before_a_search(librmu):
    h = ctypes.c_void_p()
    d = ctypes.c_double(-1.0)
    assert librmu.rmu_bm25_create(ctypes.byref(h), 1.5, 0.75, 0.25) == 0
    try:
        assert librmu.rmu_bm25_add_texts(h, b"a b\0b c\0c\0", 10, 3, None) == 0
        assert librmu.rmu_bm25_set_option(h, 8, 0) == 0 and librmu.rmu_bm25_set_option(h, 8, 1) == 0
        for bad in (2, -1):
            assert librmu.rmu_bm25_set_option(h, 8, bad) == -1, bad
            assert b"RMU_BM25_OPT_REPACK_ON_ADD" in librmu.rmu_last_error()
        assert librmu.rmu_bm25_add_texts(h, b"d\0", 2, 1, None) == 0          # on either setting an add stays host work
        assert librmu.rmu_bm25_set_option(h, 8, 0) == 0
        assert librmu.rmu_bm25_add_texts(h, b"e\0", 2, 1, None) == 0
        for what in (16, 17, 18):
            d.value = -1.0
            assert librmu.rmu_bm25_stat(h, what, ctypes.byref(d)) == 0 and d.value == 0.0, what
        for what in (6, 15, 19):
            assert librmu.rmu_bm25_stat(h, what, ctypes.byref(d)) == -1, what
        for opt in (3, 5, 7, 9, 16):
            assert librmu.rmu_bm25_set_option(h, opt, 0) == -1, opt
    finally:
        assert librmu.rmu_bm25_free(h) == 0


def test_image_stat_is_all_zeros_and_stat_keeps_its_keys(librmu):
    from ragmeup_amd.bm25 import BM25Index
    ix = BM25Index()
    try:
        assert ix.image_stat() == {"packs": 0, "splices": 0, "upload_bytes": 0}
        ix.add_texts(_tricky_corpus())
        assert set(ix.stat()) == {"docs", "vocab", "nnz", "avgdl"}
        ix.remove([0])
        assert set(ix.stat()) == {"docs", "vocab", "nnz", "avgdl", "live"}
        ix.add_texts(["one more"])
        ix.compact()
        assert set(ix.stat()) == {"docs", "vocab", "nnz", "avgdl"}
        assert ix.image_stat() == {"packs": 0, "splices": 0, "upload_bytes": 0}
    finally:
        ix.close()


def test_the_splice_kernel_is_in_the_library_without_scratch_or_lds(tmp_path, librmu):
    """found the way test_the_masked_kernel_is_in_the_library_without_scratch finds its kernels; the name carries neither of the substrings
    that test counts"""
    import re
    import shutil
    import subprocess
    from ragmeup_amd import _native
    objdump, readelf = "/opt/rocm/lib/llvm/bin/llvm-objdump", "/opt/rocm/lib/llvm/bin/llvm-readelf"
    if not (os.path.exists(objdump) and os.path.exists(readelf)):
        pytest.skip("ROCm's llvm-objdump / llvm-readelf are not installed")
    so = tmp_path / "librmu.so"
    shutil.copy(os.path.join(os.path.dirname(_native.__file__), "lib", "librmu.so"), so)
    assert subprocess.run([objdump, "--offloading", str(so)], capture_output=True, text=True, cwd=tmp_path).returncode == 0
    found = {}
    for co in sorted(tmp_path.glob("librmu.so.*gfx950")):
        notes = subprocess.run([readelf, "--notes", str(co)], capture_output=True, text=True).stdout
        for lds_bytes, name, private in re.findall(
                r"\.group_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.name:\s+(\S+)\n\s+\.private_segment_fixed_size:\s+(\d+)", notes):
            if "bm25_splice_kernel" in name:
                found[name] = (int(private), int(lds_bytes))
    assert len(found) == 1 and set(found.values()) == {(0, 0)}, found
    assert not any("bm25_topk_kernel" in n or "bm25_masked_kernel" in n for n in found)
