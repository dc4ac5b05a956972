"""Slot fork with shared, copy-on-write pages (docs/design/22-slot-fork.md) at the drop-in boundary, without a GPU: the header declares the two entry points
with the contract's argument lists, the built library exports them, CpuDecodeStore carries the methods, the copy kernel sits beside the zero kernel, and the
allocator's sharing -- host-only code -- passes its stand-alone checks, hand-written scenarios and seeded random calls beside a naive model, under
AddressSanitizer and UBSan in child processes."""
import inspect
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "krasis_amd", "csrc")

DECLS = {
    "kr_decode_slot_fork": ["s", "src", "n_dst", "dsts", "seq_len"],
    "kr_decode_slot_page_ids": ["s", "slot", "ids_out", "refs_out"],
    "kr_decode_slots_page_stride": ["s", "stride_out"],
    "kr_copy_pages": ["pool", "page_bytes", "n_pages", "page_tokens", "n_copies", "dst_pages", "src_pages", "rows", "base_offset"],
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
    # what cannot be checked is said where the caller reads it
    text = open(os.path.join(ROOT, "include", "krasis_hip.h")).read()
    assert "seq_len must therefore be the number of tokens src has consumed" in text


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
    assert list(inspect.signature(CpuDecodeStore.fork_slot).parameters) == ["self", "src", "dsts", "seq_len"]
    assert list(inspect.signature(CpuDecodeStore.slot_page_ids).parameters) == ["self", "slot"]
    assert "number of tokens src has consumed" in " ".join(CpuDecodeStore.fork_slot.__doc__.split())
    # the paged interface is what it was
    assert list(inspect.signature(CpuDecodeStore.create_slots).parameters) == ["self", "n", "max_seq", "page_tokens", "n_pages"]
    assert list(inspect.signature(CpuDecodeStore.slot_pages).parameters) == ["self"]


def test_the_copy_kernel_sits_beside_the_zero_kernel():
    """one kernel over the same device array of pools, 256 threads, written in plain C++: no inline assembly"""
    src = open(os.path.join(CSRC, "kr_multi.hip")).read()
    m = re.search(r"__global__ void __launch_bounds__\(256\) kr_multi_copy_pages_kernel\(const KrPagePoolDev\* __restrict__ pools,(.*?)\n\}\n", src, re.S)
    assert m, "kr_multi_copy_pages_kernel"
    assert "asm" not in m.group(1) and "uint4" in m.group(1)
    assert src.index("kr_multi_zero_pages_kernel") < src.index("kr_multi_copy_pages_kernel")
    assert "kr_launch_multi_copy_pages" in open(os.path.join(CSRC, "kr_multi.h")).read()
    # the pass opens with table entries, the zero launch, the copy launch -- in that order
    multi = open(os.path.join(CSRC, "kr_decode_multi.cpp")).read()
    flush = multi[multi.index("int pg_flush("):multi.index("int pg_released(")]      # to the next function
    assert flush.index("pg_upload(") < flush.index("kr_launch_multi_zero_pages(") < flush.index("kr_launch_multi_copy_pages(")


def test_the_allocator_is_still_host_only():
    code = re.sub(r"//.*", "", open(os.path.join(CSRC, "kr_page_pool.h")).read())
    assert "hip" not in code.lower()
    assert "std::vector<int32_t> refs" in code and "void share(int src, int dst, int n_entries)" in code
    # and it alone keeps the holds, the free list and the queue of mappings the device has not seen: the library calls its members
    multi = re.sub(r"//.*", "", open(os.path.join(CSRC, "kr_decode_multi.cpp")).read())
    for word in (".holds[", "pg.take(", "pg_pending"):
        assert word not in multi, word


def test_sharing_program_under_sanitizers(tmp_path):
    """share and references, the free count under shared pages, trim of one holder, the last holder freeing, copy-on-write counted in all or nothing, a
    refusal leaving table and counts untouched, a pending copy keeping its source off the free list, lowest-free-id-first order: tests/page_share_check.cpp
    with its own main, compiled alone with -fsanitize=address,undefined and run as a child process (nothing sanitized is loaded into Python)"""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "page_share_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                           "-I", CSRC, "-o", exe, os.path.join(ROOT, "tests", "page_share_check.cpp")])      # runtimes inside the program: no library order to get wrong
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert run.returncode == 0 and "page share ok" in run.stdout, run.stdout


def test_random_calls_against_a_naive_model_under_sanitizers(tmp_path):
    """4000 seeded random calls per seed on the members of KrPagePool the library calls -- reservations that append, rewind or write nothing, fork, give-backs, trims,
    release_logged, flush_plan + flushed, give-backs of entries whose copy is still queued -- beside a naive model (a set of holders per page, lowest free id by linear
    scan, a queue pruned by its own scan): table, refs, holds, n_free, n_shared, the whole queue and every log agree after each call, and row, need and have on a refusal;
    every flush plan against the model's queue; random copy queues through kr_page_copy_launches.  tests/page_pool_random_check.cpp with its own main,
    compiled alone with -fsanitize=address,undefined and run as a child process (nothing sanitized is loaded into Python)"""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "page_pool_random_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                           "-I", CSRC, "-o", exe, os.path.join(ROOT, "tests", "page_pool_random_check.cpp")])
    for seed in (1, 2, 3):
        run = subprocess.run([exe, "4000", str(seed)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert run.returncode == 0 and "page pool random ok" in run.stdout, (seed, run.stdout)
        counts = dict(zip(("reserved", "refused", "copies", "forks", "forks_refused", "pruned"), map(int, re.search(
            r"(\d+) reservations, (\d+) refused, (\d+) copy-on-write copies, (\d+) forks, (\d+) refused, (\d+) queue entries pruned", run.stdout).groups())))
        assert counts["refused"] >= 100 and counts["copies"] >= 50 and counts["refused"] < counts["reserved"] // 2, counts      # the run reached what it is about
        assert counts["forks"] >= 300 and counts["forks_refused"] >= 1 and counts["pruned"] >= 20, counts
