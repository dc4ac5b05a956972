"""Slot export and import (docs/design/38-slot-swap.md) at the drop-in boundary, without a GPU: the header declares the four entry points with the contract's
argument lists, the built library exports them, CpuDecodeStore carries the methods, what cannot be checked is said where the caller reads it, the image
description is host-only code, the two kernels are plain streaming copies, and the image layout, the header checks and the piece lists -- host-only code --
pass their stand-alone check over seeded random geometries under AddressSanitizer and UBSan in a child process."""
import inspect
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "krasis_amd", "csrc")

DECLS = {
    "kr_decode_slot_image_bytes": ["s", "seq_len", "with_sampler", "bytes_out"],
    "kr_decode_slots_export": ["s", "n", "slots", "seq_lens", "images", "image_bytes", "release"],
    "kr_decode_slots_import": ["s", "n", "slots", "images", "image_bytes", "seq_lens_out"],
    "kr_decode_slot_image_info": ["image", "bytes", "seq_len_out", "kv_fp8_out", "has_sampler_out", "geometry_out"],
}


def test_header_declares_the_entry_points():
    from krasis_amd import _lib
    text = open(os.path.join(ROOT, "include", "krasis_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name, want in DECLS.items():
        decl = re.search(r"int\s+%s\s*\(([^)]*)\)\s*;" % name, src)
        assert decl, f"{name} not declared"
        assert [a.split()[-1].lstrip("*") for a in decl.group(1).split(",")] == want, name
        assert name in _lib.SYMBOLS
    assert "void* const* images" in src and "const void* const* images" in src
    multi = open(os.path.join(CSRC, "kr_decode_multi.cpp")).read()
    for name in DECLS:
        assert re.search(r'extern "C" int %s\(' % name, multi), name
    # what cannot be checked is said where the caller reads it
    assert "seq_len must therefore be the number of tokens the slot has consumed (this cannot be checked)" in " ".join(text.split())


def test_library_exports_the_symbols():
    from krasis_amd import _lib
    if not os.path.exists(_lib.lib_path()):
        subprocess.check_call(["make", "-C", CSRC])
    lib = _lib.load_library()
    for name, want in DECLS.items():
        assert hasattr(lib, name), name
        assert len(getattr(lib, name).argtypes) == len(want), name


def test_store_methods_and_signatures():
    from krasis_amd import decode_store
    from krasis_amd.decode_store import CpuDecodeStore
    sig = lambda f: list(inspect.signature(f).parameters)
    assert sig(CpuDecodeStore.slot_image_bytes) == ["self", "seq_len"]
    assert sig(CpuDecodeStore.export_slots) == ["self", "slots", "seq_lens", "release"]
    assert inspect.signature(CpuDecodeStore.export_slots).parameters["release"].default is False
    assert sig(CpuDecodeStore.import_slots) == ["self", "slots", "images"]
    assert sig(CpuDecodeStore.export_slot) == ["self", "slot", "seq_len", "release"]
    assert inspect.signature(CpuDecodeStore.export_slot).parameters["release"].default is False
    assert sig(CpuDecodeStore.import_slot) == ["self", "slot", "image"]
    assert sig(decode_store.slot_image_info) == ["image"]
    doc = " ".join(CpuDecodeStore.export_slots.__doc__.split())
    assert "seq_len must be the number of tokens the slot has consumed (this cannot be checked)" in doc


def test_image_info_is_host_only_and_refuses_what_is_no_image():
    """kr_decode_slot_image_info needs neither a store nor a device: a hand-made image of a store without layers, and its corruptions"""
    from krasis_amd import _lib
    from krasis_amd.decode_store import slot_image_info
    if not os.path.exists(_lib.lib_path()):
        subprocess.check_call(["make", "-C", CSRC])
    head = np.zeros(16, np.uint32)
    head[:8] = [0x49534C53, 1, 1, 7, 0, 64, 100, 0]      # magic, version, E4M3, seq_len 7, no layers, hidden, vocab, no sampler
    head[8:10] = [0xDEADBEEF, 0x12345678]; head[10] = 64; head[12] = 0; head[13] = 64      # digest, total bytes, sections, table offset
    assert slot_image_info(head.view(np.uint8)) == dict(seq_len=7, kv_fp8=True, has_sampler=False, geometry=0x12345678DEADBEEF)
    assert slot_image_info(head.tobytes())["seq_len"] == 7
    assert slot_image_info(head)["seq_len"] == 7 and slot_image_info(head.reshape(4, 4))["geometry"] == 0x12345678DEADBEEF      # another dtype: the same bytes, not converted values
    for word, value in ((0, 0x49534C54), (1, 2), (10, 80), (12, 1), (13, 48)):
        bad = head.copy(); bad[word] = value
        with pytest.raises(ValueError):
            slot_image_info(bad.view(np.uint8))
    with pytest.raises(ValueError):
        slot_image_info(head.view(np.uint8)[:48])


def test_the_image_description_is_host_only():
    code = re.sub(r"//.*", "", open(os.path.join(CSRC, "kr_slot_image.h")).read())
    assert "hip" not in code.lower()
    for word in ("struct KrSlotImageHeader", "struct KrSlotSection", "struct KrSlotPiece", "kr_slot_pieces(", "kr_slot_image_check(", "KR_SLOT_PIECE_CAP"):
        assert word in code, word
    assert "kr_slot_image.h" in open(os.path.join(CSRC, "Makefile")).read()


def test_the_kernels_are_plain_streaming_copies():
    """one workgroup of 256 threads per piece, 16-byte vectors, plain C++: no inline assembly anywhere in the file; the launchers are declared beside the page
    launches and the file is part of the library"""
    src = open(os.path.join(CSRC, "kr_multi_swap.hip")).read()
    code = re.sub(r"//.*", "", src)
    for name in ("kr_multi_pack_kernel", "kr_multi_unpack_kernel"):
        assert re.search(r"__global__ void __launch_bounds__\(256\) %s\(const KrPagePoolDev\* __restrict__ pools," % name, code), name
    assert "asm" not in code and "uint4" in code and "__shared__" not in code
    head = open(os.path.join(CSRC, "kr_multi.h")).read()
    assert "kr_launch_multi_pack(" in head and "kr_launch_multi_unpack(" in head
    assert "kr_multi_swap.hip" in open(os.path.join(CSRC, "Makefile")).read()
    # export and import issue no device-wide synchronisation
    multi = re.sub(r"//.*", "", open(os.path.join(CSRC, "kr_decode_multi.cpp")).read())
    swap = multi[multi.index("KrSlotGeo swap_geo("):multi.index('extern "C" int kr_decode_slot_save(')]
    assert "hipDeviceSynchronize" not in swap and "pg_flush(" in swap and "order_after_store(" in swap and "hipHostMalloc(" in swap


def test_the_built_kernels_use_no_scratch(tmp_path):
    """the code objects of the built library: both kernels are there, for gfx950, with no private segment (nothing spilled) and no LDS"""
    import struct
    from krasis_amd import _lib
    llvm = "/opt/rocm/lib/llvm/bin"
    objcopy, readelf = os.path.join(llvm, "llvm-objcopy"), os.path.join(llvm, "llvm-readelf")
    assert os.path.exists(objcopy) and os.path.exists(readelf), "llvm-objcopy / llvm-readelf of the ROCm toolchain that built the library"
    if not os.path.exists(_lib.lib_path()):
        subprocess.check_call(["make", "-C", CSRC])
    fat = tmp_path / "fatbin"
    subprocess.check_call([objcopy, f"--dump-section=.hip_fatbin={fat}", _lib.lib_path(), str(tmp_path / "copy.so")])
    blob = fat.read_bytes()
    magic = b"__CLANG_OFFLOAD_BUNDLE__"
    objs = []
    for m in re.finditer(magic, blob):          # one bundle per translation unit: u64 entry count, then (offset, size, triple size, triple)
        p = m.start() + len(magic)
        (count,) = struct.unpack_from("<Q", blob, p)
        p += 8
        for _ in range(count):
            off, size, tsz = struct.unpack_from("<QQQ", blob, p)
            p += 24
            triple = blob[p:p + tsz].decode()
            p += tsz
            body = blob[m.start() + off:m.start() + off + size]
            if "gfx950" in triple and size and b"kr_multi_pack_kernel" in body:
                path = tmp_path / f"co_{len(objs)}.o"
                path.write_bytes(body)
                objs.append(str(path))
    assert len(objs) == 1, "the code object of kr_multi_swap.hip was not found in .hip_fatbin"
    notes = subprocess.check_output([readelf, "--notes"] + objs, text=True)
    for name in ("kr_multi_pack_kernel", "kr_multi_unpack_kernel"):
        entry = re.search(r"\.group_segment_fixed_size:\s+(\d+)(?:(?!\.name:).)*?\.name:\s+\S*%s\S*\n\s+\.private_segment_fixed_size:\s+(\d+)" % name, notes, re.S)
        assert entry, (name, notes[:2000])
        assert entry.group(1) == "0" and entry.group(2) == "0", (name, entry.groups())


def test_image_program_under_sanitizers(tmp_path):
    """layer mixes of linear attention / GQA / MLA / none, row sizes that are no multiple of 16, seq_len in {0, 1, page - 1, page, page + 1, max_seq}, pages of 32
    and 64 and flat slots, random tables with unmapped entries, ranges of 1040, 4096 and 2^20 bytes: the piece lists of consecutive ranges cover every device
    byte of the payload exactly once, never cross a page, never exceed the cap; carried out with memcpy they give the canonical image out of a flat and two
    paged placements; unpacked into a third placement and packed again, the same bytes, nothing else written; each corrupted header field is refused.
    tests/slot_image_check.cpp with its own main, compiled alone with -fsanitize=address,undefined and run as a child process (nothing sanitized is loaded
    into Python)"""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "slot_image_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                           "-I", CSRC, "-o", exe, os.path.join(ROOT, "tests", "slot_image_check.cpp")])
    for seed in (1, 2):
        run = subprocess.run([exe, "24", str(seed)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert run.returncode == 0 and "slot image ok" in run.stdout, (seed, run.stdout)
