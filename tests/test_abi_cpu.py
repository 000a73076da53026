"""CPU: librmu.so builds, loads and exports every symbol include/rmu.h declares (no compute calls)."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    src = open(os.path.join(ROOT, "include", "rmu.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(rmu_[a-z0-9_]+)\s*\(", src)))


def test_header_symbols_exported(librmu):
    names = _declared()
    assert len(names) >= 18
    missing = [n for n in names if not hasattr(librmu, n)]
    assert not missing, f"librmu.so does not export {missing}"


def test_binding_lists_every_declared_symbol():
    from ragmeup_amd import _native
    assert sorted(_native.SYMBOLS) == _declared()


def test_version_and_error_strings(librmu):
    assert b"gfx950" in librmu.rmu_version()
    assert isinstance(librmu.rmu_last_error(), bytes)


def test_invalid_arguments_fail_without_gpu(librmu):
    """Argument validation happens before any HIP call, so it is testable on the GPU-less builder."""
    import ctypes
    h = ctypes.c_void_p()
    assert librmu.rmu_index_create(None, 384, 0, 0) == -1
    assert librmu.rmu_index_create(ctypes.byref(h), 0, 0, 0) == -1
    assert librmu.rmu_index_create(ctypes.byref(h), 4096, 0, 0) == -1
    assert librmu.rmu_index_create(ctypes.byref(h), 384, 7, 0) == -1
    assert b"metric" in librmu.rmu_last_error()
    assert librmu.rmu_index_search(None, None, 1, 10, 0, 0, None, None, 0) == -1
    assert librmu.rmu_topk_merge(None, None, 1, 1, 10, 0, None, None, 0) == -1
    v = ctypes.c_double(0.0)
    assert librmu.rmu_probe_mfma_rate(0, 0, 100, None) == -1
    assert librmu.rmu_probe_mfma_rate(2, 0, 100, ctypes.byref(v)) == -1
    assert librmu.rmu_probe_mfma_rate(1, 1, 100, ctypes.byref(v)) == -1       # (the LDS / DMA skeleton is the f16 kernel's)
    assert librmu.rmu_probe_mfma_rate(0, 0, 0, ctypes.byref(v)) == -1


def test_product_never_imports_the_oracle():
    """The oracle is test infrastructure: nothing under ragmeup_amd/ may import, load or exec it."""
    pkg = os.path.join(ROOT, "ragmeup_amd")
    for dp, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                txt = open(os.path.join(dp, f), errors="replace").read()
                assert not re.search(r"^\s*(from|import)\s+oracle\b", txt, flags=re.M), f
                assert "liboracle" not in txt and "oracle/" not in txt.replace("the oracle/", ""), f


def test_header_is_plain_c_and_the_c_example_links(tmp_path, librmu):
    """include/rmu.h must be consumable by a C compiler (the boundary is a C ABI, not a C++ one), and a plain-C program
    must link against librmu.so with nothing but -lrmu (no execution here: the library needs a GPU)."""
    import os
    import shutil
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    gcc = shutil.which("gcc")
    assert gcc, "gcc is part of the build image"
    probe = tmp_path / "probe.c"
    probe.write_text('#include "rmu.h"\nint main(void) { return rmu_version() == 0; }\n')
    subprocess.run([gcc, "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(root, "include"), str(probe)],
                   check=True, capture_output=True)
    libdir = os.path.join(root, "ragmeup_amd", "lib")
    exe = tmp_path / "flat_search"
    r = subprocess.run([gcc, "-std=c99", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(root, "include"),
                        os.path.join(root, "examples", "flat_search.c"), "-L", libdir, "-lrmu", "-Wl,-rpath," + libdir,
                        "-Wl,--allow-shlib-undefined", "-lm", "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert exe.exists()


def test_the_library_reads_tuning_switches_only_behind_the_master_switch():
    """Every RMU_* environment switch of librmu goes through rmu_env(), which answers only when RMU_TUNING=1 is set: a stray variable in
    a server's environment cannot change which kernels run."""
    import glob
    import re
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ragmeup_amd", "csrc")
    direct = []
    for f in glob.glob(os.path.join(csrc, "*.hip")) + glob.glob(os.path.join(csrc, "*.h")):
        for m in re.finditer(r'(?<![_a-z])getenv\("(\w+)"\)', open(f).read()):
            if m.group(1) != "RMU_TUNING":
                direct.append((os.path.basename(f), m.group(1)))
    assert direct == []
    common = open(os.path.join(csrc, "rmu_common.h")).read()
    assert 'inline const char* rmu_env(const char* name)' in common and 'getenv("RMU_TUNING")' in common


def test_the_product_library_carries_only_the_kernels_it_takes():
    """the superseded forms of the screening kernel (scan_screen_kernel, scan_screen_lean_kernel,
    scan_screen_lean2_kernel, the K-split / 128-queries-per-wave experiments) are retired (profiles/r04_ab_screen_forms.txt, NOTES_r01_r05.md 4.5)
    and the round-1/2 encoder kernels are retired; the product library's symbol table names scan_screen_lean3_kernel (three geometries, each in its inner-product and its
    L2 form -- round 5 -- and, round 6, each of those with the 128-key candidate slots of 32 < k <= 104) and nothing else of that family."""
    import re
    import shutil
    import subprocess
    from ragmeup_amd import _native
    nm = shutil.which("nm") or "/opt/rocm/lib/llvm/bin/llvm-nm"
    out = subprocess.run([nm, "-C", _native.SO_PATH], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    screen = sorted(set(re.findall(r"scan_screen\w*kernel<[^>]*>", out.stdout)))
    assert screen == [f"scan_screen_lean3_kernel<0, {g}, {l2}, {deep}>" for g in ("4, 0", "4, 1", "8, 0") for l2 in (0, 1) for deep in ("false", "true")], screen
    for gone in ("k_ffn_fused", "k_attention<", "k_attn4", "k_gemm_mid"):
        assert gone not in out.stdout, gone
    # the exact scan and its gathered form: the instantiations the library dispatches to, under the names tools/summarize_profiles.py and the
    # committed profiles match on (Cfg<D, WQ, CKF, RING, CAP, NCHECK, EXP, LA, NT> / SCfg<D, WQ, CKF, CAP, NCHECK>)
    topk = sorted(set(re.findall(r"scan_topk_kernel<[^>]*>", out.stdout)))
    assert topk == [f"scan_topk_kernel<(anonymous namespace)::Cfg<{d}, {c}>" for d in (192, 384, 768) for c in TOPK_CFGS], topk
    subset = sorted(set(re.findall(r"scan_subset_kernel<[^>]*>", out.stdout)))
    assert subset == [f"scan_subset_kernel<(anonymous namespace)::SCfg<{d}>" for d in SUBSET_CFGS], subset


TOPK_CFGS = ("1, 48, 3, 64, 1, 0, 0, 0", "1, 48, 3, 64, 1, 0, 0, 1", "2, 48, 2, 128, 2, 0, 1, 0", "2, 96, 3, 64, 1, 0, 0, 0",
             "2, 96, 3, 64, 1, 0, 0, 1", "4, 96, 2, 128, 2, 0, 1, 0", "4, 96, 4, 64, 1, 0, 1, 0")      # x three widths = 21
SUBSET_CFGS = ("192, 1, 48, 64, 1", "192, 4, 32, 128, 2", "192, 4, 32, 64, 1", "384, 1, 48, 64, 1", "384, 4, 32, 128, 2", "384, 4, 96, 64, 1",
               "768, 1, 48, 64, 1", "768, 4, 32, 128, 2", "768, 4, 96, 64, 1")



def test_no_device_wide_synchronisation_and_every_entry_point_in_relaxed_capture_mode():
    """(round 6; profiles/r06_capture_probe.txt) A hipDeviceSynchronize, a synchronous hipMemcpy / hipMemset on ANY thread invalidates a
    hipGraph capture running on another thread -- the reference's LLM captures in the same process (server/RAGHelper_local.py:42-105) --
    and a thread in the default capture-interaction mode does so with most synchronous calls.  The library's product sources therefore
    (1) never call them (the debug-counter dumps under RMU_DEBUG_KERNELS / RMU_SCAN_EXP aside) and (2) open every exported entry point
    that reaches HIP with RMU_ENTRY() (relaxed mode for the duration of the call); its own captures are still taken one at a time."""
    import glob
    import os
    import re
    src = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ragmeup_amd", "csrc")
    bare = []
    for path in sorted(glob.glob(os.path.join(src, "*.hip")) + glob.glob(os.path.join(src, "*.h"))):
        text = open(path, encoding="utf-8").read()
        # debug-only regions: everything between #ifdef RMU_DEBUG_KERNELS and its #endif / #else, and the RMU_SCAN_EXP counter dump
        text = re.sub(r"#ifdef RMU_DEBUG_KERNELS.*?#(?:endif|else)", lambda m: "\n" * m.group(0).count("\n"), text, flags=re.S)
        for i, ln in enumerate(text.split("\n")):
            code = ln.split("//")[0]
            if re.search(r"\bhipDeviceSynchronize\(|\bhipMemcpy\(|\bhipMemset\(|\bhipMemcpy2D\(", code) and "dbg" not in code:
                bare.append(f"{os.path.basename(path)}:{i + 1}: {code.strip()[:80]}")
    assert not bare, bare
    common = open(os.path.join(src, "rmu_common.h"), encoding="utf-8").read()
    assert "hipThreadExchangeStreamCaptureMode" in common and "#define RMU_ENTRY()" in common
    # every `extern "C" int rmu_*` with a body of its own lines that touches HIP starts with RMU_ENTRY()
    missing = []
    for name in ("rmu_api.hip", "bert.hip", "rmu_comm.hip"):
        text = open(os.path.join(src, name), encoding="utf-8").read()
        for m in re.finditer(r'^extern "C" int (rmu_\w+)\([^;{]*\)\s*\{\n(.*?)^\}', text, flags=re.S | re.M):
            fn, body = m.group(1), m.group(2)
            if re.search(r"\bhip[A-Z]\w+\(|ensure_stream|hipLaunchKernelGGL|nccl[A-Z]", body) and "RMU_ENTRY();" not in body.split("\n")[0]:
                missing.append(fn)
    assert missing == [], missing
    bert = open(os.path.join(src, "bert.hip"), encoding="utf-8").read()
    cap = bert.index("hipStreamBeginCapture(")
    assert "rmu_capture_mutex()" in bert[cap - 400:cap]
    assert re.search(r"inline std::mutex& rmu_capture_mutex\(\)", common)


def test_no_kernel_of_the_product_library_spills_to_scratch(tmp_path):
    """(round 6) Two uniform `if`s added to k_ffn3 for an A/B experiment cost the register allocator 196 bytes of scratch per lane: +4.8 GB of
    HBM traffic per forward and 3.05 -> 3.30 ms per launch, found only because a PMC table looked wrong.  The code objects inside librmu.so
    carry every kernel's resources: none of the hot kernels may have a private (scratch) segment."""
    import re
    import shutil
    import subprocess
    from ragmeup_amd import _native
    objdump = "/opt/rocm/lib/llvm/bin/llvm-objdump"
    readelf = "/opt/rocm/lib/llvm/bin/llvm-readelf"
    if not (os.path.exists(objdump) and os.path.exists(readelf)):
        import pytest
        pytest.skip("ROCm's llvm-objdump / llvm-readelf are not installed")
    so = tmp_path / "librmu.so"
    # the PRODUCT library, whatever RMU_LIB selects for this process (`make asan-test` runs the suite against librmu_asan.so, whose device code is
    # compiled with -g and the sanitizer flags: its register allocation is not the shipped one -- the 768-wide exact-scan instantiations keep 20-36
    # bytes of scratch there)
    product = os.path.join(os.path.dirname(_native.__file__), "lib", "librmu.so")
    shutil.copy(product if os.path.exists(product) else _native.SO_PATH, so)
    r = subprocess.run([objdump, "--offloading", str(so)], capture_output=True, text=True, cwd=tmp_path)
    assert r.returncode == 0, r.stderr[-2000:]
    found, spilled = 0, []
    for co in sorted(tmp_path.glob("librmu.so.*gfx950")):
        notes = subprocess.run([readelf, "--notes", str(co)], capture_output=True, text=True).stdout
        for name, scratch in re.findall(r"\.name:\s+(\S+)\n\s+\.private_segment_fixed_size:\s+(\d+)", notes):
            found += 1
            if int(scratch) != 0:
                spilled.append((name[:70], int(scratch)))
    assert found > 40, found                                   # the metadata was really read
    hot = [s for s in spilled if re.search(r"k_ffn3|k_gemm3|k_attn3|k_gemm|scan_screen_lean3|scan_topk|k_qa|k_rescore|merge_select", s[0])]
    assert hot == [], hot


def _csrc_sources():
    """name -> text of every csrc/*.hip and *.h, `//` comments blanked (offsets keep their lines)."""
    import glob
    csrc = os.path.join(ROOT, "ragmeup_amd", "csrc")
    out = {}
    for path in sorted(glob.glob(os.path.join(csrc, "*.hip")) + glob.glob(os.path.join(csrc, "*.h"))):
        text = open(path, encoding="utf-8").read()
        out[os.path.basename(path)] = re.sub(r"//[^\n]*", "", text)
    return out


def _block(text, open_brace):
    """The text of the brace block that opens at text[open_brace]."""
    depth = 0
    for i in range(open_brace, len(text)):
        depth += text[i] == "{"
        depth -= text[i] == "}"
        if depth == 0:
            return text[open_brace:i + 1]
    raise AssertionError("unbalanced braces")


def _enclosing(text, pos, header):
    """Name (group 1 of `header`, a regex that ends at an opening brace) of the innermost block that holds text[pos]."""
    name = None
    for m in re.finditer(header, text[:pos]):
        if m.group(1) not in ("if", "for", "while", "switch", "catch") and m.end() - 1 + len(_block(text, m.end() - 1)) > pos:
            name = m.group(1)
    return name


_FN = r"\b(\w+)\s*\([^;{}]*\)\s*(?:const\s*)?\{"
_STRUCT = r"\bstruct\s+(\w+)[^;{}()]*\{"


def test_host_plumbing_exists_once():
    """One grow-only device buffer, one grow-only pinned buffer, one HIP error path, one runtime-down flag (csrc/rmu_host.h; the flag and the
    thread's message live in rmu_api.hip): a unit that brings a copy of its own fails here."""
    src = _csrc_sources()
    dev, pin, macros, setters, decls, guards = [], [], [], [], [], []
    for name, text in src.items():
        for m in re.finditer(r"\bhipMalloc\(", text):
            owner = _enclosing(text, m.start(), _STRUCT)      # (a member function: the encoder's free ensure_* functions grow a model's arrays)
            if owner and (_enclosing(text, m.start(), _FN) or "").startswith("ensure"):
                dev.append((name, owner))
        for m in re.finditer(r"\bhipHostMalloc\(", text):
            pin.append((name, _enclosing(text, m.start(), _STRUCT), _enclosing(text, m.start(), _FN)))
        macros += [(name, m.group(1)) for m in re.finditer(r"^[ \t]*#[ \t]*define[ \t]+(\w+_TRY)\b", text, flags=re.M)]
        for m in re.finditer(r"\brmu_set_error_\(\s*\w+\.c_str\(\)\s*\)", text):
            setters.append((name, _enclosing(text, m.start(), _FN)))
        decls += [name for m in re.finditer(r"\bvoid\s+rmu_set_error_\s*\([^)]*\)\s*;", text)]
        for m in re.finditer(r"~(\w+)\s*\(\s*\)\s*\{", text):
            if re.search(r"\w*down\w*\s*=\s*true", _block(text, m.end() - 1)):
                guards.append((name, m.group(1)))
    assert dev == [("rmu_host.h", "RmuDevBuf")], dev
    # the two allowed other sites are no growable buffers: the index's single pinned word and the encoder's fixed staging
    assert sorted(set(pin)) == [("bert.hip", None, "host_staging_locked"), ("rmu_api.hip", "Tls", "ensure_hflag"),
                                ("rmu_host.h", "RmuPinBuf", "ensure")], pin
    assert macros == [("rmu_host.h", "RMU_HIP_TRY")], macros
    assert setters == [("rmu_host.h", "rmu_fail")], setters
    assert decls == ["rmu_host.h"], decls
    assert guards == [("rmu_api.hip", "RuntimeGuard")], guards
    # no unit forwards to the one error path through a wrapper of its own
    wrappers = [(name, m.group(1)) for name, text in src.items()
                for m in re.finditer(r"\bint\s+(\w*fail)\s*\([^)]*\)\s*\{[^}]*\brmu_(?:fail|set_error_)\(", text) if m.group(1) != "rmu_fail"]
    assert wrappers == [], wrappers
