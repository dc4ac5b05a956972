"""Verify and commit over device slots (docs/design/18-multi-verify.md) at the drop-in boundary, without a GPU: the header declares the three entry
points with the contract's argument lists, the built library exports them, CpuDecodeStore carries the methods, and the drafting index has one copy."""
import inspect
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "krasis_amd", "csrc")

DECLS = {
    "kr_decode_verify_multi": ["s", "n", "slots", "counts", "tokens", "positions", "greedy_out", "n_match_out", "stream"],
    "kr_decode_commit_multi": ["s", "n_keep"],
    "kr_decode_generate_multi_lookup": ["s", "n", "slots", "contexts", "n_context", "first_tokens", "start_positions", "max_tokens", "max_draft", "ngram_max",
                                        "stop_ids", "n_stop", "tokens_out", "n_out", "n_passes_out", "n_accepted_out", "stream"],
}


def test_header_declares_the_entry_points():
    from krasis_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "krasis_hip.h")).read(), flags=re.S)
    for name, want in DECLS.items():
        decl = re.search(r"int\s+%s\s*\(([^)]*)\)\s*;" % name, src)
        assert decl, f"{name} not declared"
        assert [a.split()[-1].lstrip("*") for a in decl.group(1).split(",")] == want, name
        assert name in _lib.SYMBOLS


def test_library_exports_the_symbols():
    from krasis_amd import _lib
    if not os.path.exists(_lib.lib_path()):
        subprocess.check_call(["make", "-C", CSRC])
    lib = _lib.load_library()
    for name, want in DECLS.items():
        assert hasattr(lib, name), name
        assert len(getattr(lib, name).argtypes) == len(want), name


def test_store_methods_and_signatures():
    from krasis_amd.decode_store import LOOKUP_MAX_DRAFT, CpuDecodeStore
    assert list(inspect.signature(CpuDecodeStore.verify_multi).parameters) == ["self", "slots", "token_lists", "positions"]
    assert list(inspect.signature(CpuDecodeStore.commit_multi).parameters) == ["self", "n_keep"]
    gen = inspect.signature(CpuDecodeStore.generate_multi_lookup)
    assert list(gen.parameters) == ["self", "slots", "first_tokens", "start_positions", "max_tokens", "contexts", "max_draft", "ngram_max", "stop_ids"]
    assert gen.parameters["contexts"].default is None and gen.parameters["max_draft"].default == LOOKUP_MAX_DRAFT and gen.parameters["stop_ids"].default == ()


def test_the_drafting_index_has_one_copy():
    """LookupIndex lives in kr_lookup_index.h; both generation loops include it and neither defines its own"""
    defs = [f for f in sorted(os.listdir(CSRC)) if f.endswith((".h", ".cpp", ".hip")) and "struct LookupIndex" in open(os.path.join(CSRC, f)).read()]
    assert defs == ["kr_lookup_index.h"]
    for f in ("kr_decode_spec.cpp", "kr_decode_multi.cpp"):
        assert '#include "kr_lookup_index.h"' in open(os.path.join(CSRC, f)).read(), f
    assert "kr_lookup_index.h" in open(os.path.join(CSRC, "Makefile")).read()
