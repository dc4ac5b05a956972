"""Paged sequence slots (docs/design/21-paged-slots.md) at the drop-in boundary, without a GPU: the header declares the three entry points with the
contract's argument lists, the built library exports them, CpuDecodeStore carries the methods, the kernels take paging as a template parameter, and the
page allocator -- a host-only header -- passes its stand-alone check under AddressSanitizer and UBSan in a child process."""
import inspect
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "krasis_amd", "csrc")

DECLS = {
    "kr_decode_slots_create_paged": ["s", "n_slots", "max_seq", "page_tokens", "n_pages", "bytes_out"],
    "kr_decode_slot_trim": ["s", "slot", "seq_len"],
    "kr_decode_slots_pages": ["s", "page_tokens_out", "n_pages_out", "n_free_out", "per_slot_out"],
}


def test_header_declares_the_entry_points():
    from krasis_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "krasis_hip.h")).read(), flags=re.S)
    for name, want in DECLS.items():
        decl = re.search(r"int\s+%s\s*\(([^)]*)\)\s*;" % name, src)
        assert decl, f"{name} not declared"
        assert [a.split()[-1].lstrip("*") for a in decl.group(1).split(",")] == want, name
        assert name in _lib.SYMBOLS
    multi = open(os.path.join(CSRC, "kr_decode_multi.cpp")).read()
    for name in DECLS:
        assert re.search(r'extern "C" int %s\(' % name, multi), name


def test_library_exports_the_symbols():
    from krasis_amd import _lib
    if not os.path.exists(_lib.lib_path()):
        subprocess.check_call(["make", "-C", CSRC])
    lib = _lib.load_library()
    for name, want in DECLS.items():
        assert hasattr(lib, name), name
        assert len(getattr(lib, name).argtypes) == len(want), name


def test_store_methods_and_signatures():
    from krasis_amd.decode_store import CpuDecodeStore
    create = inspect.signature(CpuDecodeStore.create_slots)
    assert list(create.parameters) == ["self", "n", "max_seq", "page_tokens", "n_pages"]
    assert create.parameters["page_tokens"].default is None and create.parameters["n_pages"].default is None
    assert list(inspect.signature(CpuDecodeStore.trim_slot).parameters) == ["self", "slot", "seq_len"]
    assert list(inspect.signature(CpuDecodeStore.slot_pages).parameters) == ["self"]


def test_one_without_the_other_is_a_value_error():
    """page_tokens and n_pages go together: refused in Python, before the library is asked"""
    from krasis_amd.decode_store import CpuDecodeStore
    st = CpuDecodeStore.__new__(CpuDecodeStore)
    st._need = lambda: None
    for kw in (dict(page_tokens=32), dict(n_pages=4)):
        with pytest.raises(ValueError):
            st.create_slots(2, 64, **kw)
    st._h = None      # __del__ has nothing to free


def test_paging_is_a_template_parameter_of_the_four_kernels():
    """the flat instantiations are the parent's code: paging is compiled in or out, never tested at run time inside the loops"""
    src = open(os.path.join(CSRC, "kr_multi.hip")).read()
    for kernel in ("kr_multi_gqa_prep_kernel", "kr_multi_gqa_attn_kernel", "kr_multi_mla_prep_kernel", "kr_multi_mla_attn_kernel"):
        m = re.search(r"template <([^>]*)>\s*__global__ void __launch_bounds__\(\d+\) %s\(" % kernel, src)
        assert m and "bool PAGED" in m.group(1), kernel
    for struct in ("KrMultiGqaArgs", "KrMultiMlaArgs"):
        body = re.search(r"struct %s \{(.*?)\n\};" % struct, open(os.path.join(CSRC, "kr_multi.h")).read(), re.S).group(1)
        assert "const int* page_table; int page_stride, page_shift;" in body, struct


def test_the_allocator_is_host_only_and_in_the_build():
    src = open(os.path.join(CSRC, "kr_page_pool.h")).read()
    code = re.sub(r"//.*", "", src)
    assert "hip" not in code.lower()
    assert "kr_page_pool.h" in open(os.path.join(CSRC, "Makefile")).read()
    assert '#include "kr_page_pool.h"' in open(os.path.join(CSRC, "kr_decode_internal.h")).read()


def test_allocator_program_under_sanitizers(tmp_path):
    """all-or-nothing reservation, lowest id first, trim, release of call-mapped pages only, exhaustion: tests/page_pool_check.cpp with its own main,
    compiled alone with -fsanitize=address,undefined and run as a child process (nothing sanitized is loaded into Python)"""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "page_pool_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                           "-I", CSRC, "-o", exe, os.path.join(ROOT, "tests", "page_pool_check.cpp")])      # runtimes inside the program: no library order to get wrong
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert run.returncode == 0 and "page pool ok" in run.stdout, run.stdout
