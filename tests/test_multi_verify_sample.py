"""Exact sampled speculation over device slots (docs/design/19-multi-verify-sample.md) at the drop-in boundary, without a GPU: the header declares the
four entry points with the contract's argument lists, the built library exports them, CpuDecodeStore carries the three new methods, and the signatures
the greedy verify pinned are as they were."""
import inspect
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "krasis_amd", "csrc")

DECLS = {
    "kr_decode_verify_multi_sample": ["s", "n", "slots", "counts", "tokens", "positions", "sampled_out", "n_match_out", "stream"],
    "kr_decode_generate_multi_lookup_sample": ["s", "n", "slots", "contexts", "n_context", "first_tokens", "start_positions", "max_tokens", "max_draft",
                                               "ngram_max", "temperature", "top_k", "top_p", "presence_penalty", "rng_seeds", "stop_ids", "n_stop",
                                               "tokens_out", "n_out", "n_passes_out", "n_accepted_out", "stream"],
    "kr_decode_slot_sampler_get": ["s", "slot", "seen_out", "rng_out"],
    "kr_sample_runs": ["logits", "n", "counts", "tokens", "vocab", "temperature", "top_k", "top_p", "presence_penalty", "seen", "rng_state", "n_keep",
                       "ids_out", "n_match_out", "force_loop"],
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
    assert list(inspect.signature(CpuDecodeStore.verify_multi_sample).parameters) == ["self", "slots", "token_lists", "positions"]
    gen = inspect.signature(CpuDecodeStore.generate_multi_lookup_sample)
    assert list(gen.parameters) == ["self", "slots", "first_tokens", "start_positions", "max_tokens", "contexts", "max_draft", "ngram_max", "stop_ids",
                                    "temperature", "top_k", "top_p", "presence_penalty", "rng_seeds"]
    assert gen.parameters["contexts"].default is None and gen.parameters["max_draft"].default == LOOKUP_MAX_DRAFT
    assert gen.parameters["ngram_max"].default == 3 and gen.parameters["stop_ids"].default == ()
    assert all(gen.parameters[p].default is None for p in ("temperature", "top_k", "top_p", "presence_penalty", "rng_seeds"))
    assert list(inspect.signature(CpuDecodeStore.slot_sampler_state).parameters) == ["self", "slot"]


def test_the_greedy_signatures_are_as_they_were():
    from krasis_amd.decode_store import LOOKUP_MAX_DRAFT, CpuDecodeStore
    assert list(inspect.signature(CpuDecodeStore.verify_multi).parameters) == ["self", "slots", "token_lists", "positions"]
    assert list(inspect.signature(CpuDecodeStore.commit_multi).parameters) == ["self", "n_keep"]
    gen = inspect.signature(CpuDecodeStore.generate_multi_lookup)
    assert list(gen.parameters) == ["self", "slots", "first_tokens", "start_positions", "max_tokens", "contexts", "max_draft", "ngram_max", "stop_ids"]
    assert gen.parameters["contexts"].default is None and gen.parameters["max_draft"].default == LOOKUP_MAX_DRAFT and gen.parameters["stop_ids"].default == ()


def test_the_generation_loop_has_one_copy():
    """the four generation entry points over slots are one function: the drafting call and the loop over the rows still generating each appear once in
    the file, in the same internal function, and the body of every entry point returns through that function"""
    src = open(os.path.join(CSRC, "kr_decode_multi.cpp")).read()
    assert src.count(".draft(max_draft, draft)") == 1
    assert len(re.findall(r"\b(?:while|for)\s*\([^\n]*\bact\.(?:empty|size)\(\)", src)) == 1      # one loop walks the active rows
    loop_at = src.index("while (!act.empty())")
    starts = {m.start(): m.group(1) for m in re.finditer(r"^\w[\w:<>*& ]* [*&]*(\w+)\(", src, flags=re.M)}      # functions defined in column 0

    def owner(at):
        return starts[max(p for p in starts if p < at)]

    loop = owner(loop_at)
    assert owner(src.index(".draft(max_draft, draft)")) == loop
    entries = ["kr_decode_generate_multi", "kr_decode_generate_multi_sample", "kr_decode_generate_multi_lookup", "kr_decode_generate_multi_lookup_sample"]
    for name in entries:
        body = re.search(r'extern "C" int %s\(.*?\)\s*\{(.*?)\n\}\n' % name, src, flags=re.S)
        assert body, name
        assert len(re.findall(r"\breturn %s\(" % loop, body.group(1))) == 1, name
    assert len(re.findall(r"\b%s\(" % loop, src)) == len(entries) + 1      # its definition and those four calls
