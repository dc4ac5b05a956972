"""The multi-token extend of device slots (kr_decode_extend_multi, docs/design/17-multi-extend.md) at the drop-in boundary, without a GPU: the
header declares the entry point and its token limit, the built library exports it, and CpuDecodeStore carries extend_multi / prefill_slot."""
import inspect
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    src = open(os.path.join(ROOT, "include", "krasis_hip.h")).read()
    return re.sub(r"/\*.*?\*/", "", src, flags=re.S)


def test_header_declares_the_entry_point_and_the_limit():
    from krasis_amd import _lib
    src = _header()
    m = re.search(r"#define\s+KR_EXTEND_MAX_TOKENS\s+(\d+)", src)
    assert m, "KR_EXTEND_MAX_TOKENS not defined in include/krasis_hip.h"
    assert int(m.group(1)) == _lib.KR_EXTEND_MAX_TOKENS == 1024
    decl = re.search(r"int\s+kr_decode_extend_multi\s*\(([^)]*)\)\s*;", src)
    assert decl, "kr_decode_extend_multi not declared"
    args = [a.strip() for a in decl.group(1).split(",")]
    assert [a.split()[-1].lstrip("*") for a in args] == ["s", "n", "slots", "counts", "tokens", "positions", "next_out", "logits_out", "sample", "stream"]
    assert "kr_decode_extend_multi" in _lib.SYMBOLS


def test_library_exports_the_symbol():
    from krasis_amd import _lib
    if not os.path.exists(_lib.lib_path()):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "krasis_amd", "csrc")])
    lib = _lib.load_library()
    assert hasattr(lib, "kr_decode_extend_multi")
    assert len(lib.kr_decode_extend_multi.argtypes) == 10


def test_store_methods_and_signatures():
    from krasis_amd.decode_store import CpuDecodeStore
    ext = inspect.signature(CpuDecodeStore.extend_multi)
    assert list(ext.parameters) == ["self", "slots", "token_lists", "positions", "logits", "sample"]
    assert ext.parameters["logits"].default is False and ext.parameters["sample"].default is False
    pre = inspect.signature(CpuDecodeStore.prefill_slot)
    assert list(pre.parameters) == ["self", "slot", "tokens", "start_pos", "chunk"]
    assert pre.parameters["start_pos"].default == 0 and pre.parameters["chunk"].default is None


def test_prefill_slot_is_plain_python_over_extend_multi():
    """chunking and argument checks happen before any native call: a stand-in for extend_multi sees the chunks"""
    from krasis_amd.decode_store import CpuDecodeStore
    calls = []

    class Stub:
        def extend_multi(self, slots, token_lists, positions, logits=False, sample=False):
            calls.append((list(slots), [list(t) for t in token_lists], list(positions)))
            return [len(calls)]

    toks = list(range(21))
    assert CpuDecodeStore.prefill_slot(Stub(), 3, toks, start_pos=5, chunk=8) == 3
    assert calls == [([3], [toks[0:8]], [5]), ([3], [toks[8:16]], [13]), ([3], [toks[16:21]], [21])]
    for bad in (dict(tokens=[], chunk=8), dict(tokens=[1], chunk=0), dict(tokens=[1], chunk=1025)):
        with pytest.raises(ValueError):
            CpuDecodeStore.prefill_slot(Stub(), 0, bad["tokens"], chunk=bad["chunk"])
