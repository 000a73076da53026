"""Wide rows (769..3072 dimensions, scan_wide.hip): what can be checked without a GPU -- the constants, the argument validation that runs
before any HIP call, the instantiations the library carries, and that none of them has a scratch segment."""
import ctypes
import os
import re
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

# the dispatch table of scan_wide.hip (with_wcfg): WCfg<WQ, CKF, RING, CAP, NCHECK, NT>
WIDE_CFGS = ("1, 32, 3, 64, 1, 0", "1, 32, 3, 64, 1, 1", "2, 16, 3, 120, 4, 0", "2, 32, 3, 64, 1, 0", "2, 32, 3, 64, 1, 1", "4, 32, 3, 64, 1, 0")


def test_constants_of_the_binding_and_the_header():
    from ragmeup_amd import _native
    assert _native.MAX_DIM_WIDE == 3072 and _native.MAX_DIM == 768 and _native.OPT_WIDE_SCAN == 6
    hdr = open(os.path.join(ROOT, "include", "rmu.h"), encoding="utf-8").read()
    assert re.search(r"^#define RMU_MAX_DIM_WIDE 3072\b", hdr, flags=re.M)
    assert re.search(r"^#define RMU_OPT_WIDE_SCAN 6\b", hdr, flags=re.M)
    assert re.search(r"^#define RMU_MAX_DIM 768\b", hdr, flags=re.M)


def test_widths_the_index_refuses_fail_without_a_gpu(librmu):
    h = ctypes.c_void_p()
    assert librmu.rmu_index_create(ctypes.byref(h), 3073, 0, 0) == -1
    assert b"3072" in librmu.rmu_last_error()
    assert librmu.rmu_index_create(ctypes.byref(h), 1024, 2, 0) == -1           # RMU_METRIC_L2SQ: no wide L2 index
    assert b"L2" in librmu.rmu_last_error()
    assert librmu.rmu_index_create(ctypes.byref(h), 768, 2, 0) == -1            # ... and the narrow one's limit reads as it did
    assert b"dim must be <= 767" in librmu.rmu_last_error()
    assert not h.value


def test_the_library_carries_the_wide_kernels_its_dispatch_table_names(librmu):
    from ragmeup_amd import _native
    nm = shutil.which("nm") or "/opt/rocm/lib/llvm/bin/llvm-nm"
    out = subprocess.run([nm, "-C", _native.SO_PATH], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    wide = sorted(set(re.findall(r"scan_wide_kernel<[^>]*>", out.stdout)))
    assert wide == [f"scan_wide_kernel<(anonymous namespace)::WCfg<{c}>" for c in WIDE_CFGS], wide
    src = open(os.path.join(ROOT, "ragmeup_amd", "csrc", "scan_wide.hip"), encoding="utf-8").read()
    table = sorted(set(re.findall(r"= WCfg<([^>]*)>;", src)))
    assert table == sorted(WIDE_CFGS), table


def test_no_wide_kernel_has_a_scratch_segment(librmu, tmp_path):
    """As test_no_kernel_of_the_product_library_spills_to_scratch: the code objects' notes, on the product library."""
    import pytest
    from ragmeup_amd import _native
    objdump = "/opt/rocm/lib/llvm/bin/llvm-objdump"
    readelf = "/opt/rocm/lib/llvm/bin/llvm-readelf"
    if not (os.path.exists(objdump) and os.path.exists(readelf)):
        pytest.skip("ROCm's llvm-objdump / llvm-readelf are not installed")
    so = tmp_path / "librmu.so"
    product = os.path.join(os.path.dirname(_native.__file__), "lib", "librmu.so")
    shutil.copy(product if os.path.exists(product) else _native.SO_PATH, so)
    r = subprocess.run([objdump, "--offloading", str(so)], capture_output=True, text=True, cwd=tmp_path)
    assert r.returncode == 0, r.stderr[-2000:]
    seen = {}
    for co in sorted(tmp_path.glob("librmu.so.*gfx950")):
        notes = subprocess.run([readelf, "--notes", str(co)], capture_output=True, text=True).stdout
        for name, scratch in re.findall(r"\.name:\s+(\S+)\n\s+\.private_segment_fixed_size:\s+(\d+)", notes):
            if "scan_wide_kernel" in name:
                seen[name] = int(scratch)
    assert len(seen) == len(WIDE_CFGS), sorted(seen)
    assert all(v == 0 for v in seen.values()), seen
