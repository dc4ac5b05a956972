"""The formulas of the exact arithmetic are stated once, in krasis_amd/csrc/kr_exact_dev.h (docs/design/02-numerics.md, "One definition per formula"):
source checks, without a GPU.  A kernel that restates the hsum tree or the softplus gate instead of calling the header fails here."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "krasis_amd", "csrc")
HEADER = "kr_exact_dev.h"

# the per-file helpers the header replaced
OLD_NAMES = ("kr_m_hsum8", "kr_m_sumsq8", "kr_pfm_hsum8", "kr_pfm_sumsq8", "kr_lc_sumsq8", "gg_hsum8", "kr_mla_hsum8", "kr_sumsq_chain8")


def sources():
    """name -> text of every source file of the library, `//` comments removed"""
    out = {}
    for name in sorted(os.listdir(CSRC)):
        if name.endswith((".hip", ".h", ".cpp", ".inc")):
            out[name] = re.sub(r"//.*", "", open(os.path.join(CSRC, name)).read())
    return out


def files_with(pattern):
    return [name for name, text in sources().items() if re.search(pattern, text)]


def test_the_header_is_there_and_in_the_build():
    assert HEADER in sources()
    hdrs = re.search(r"^HDRS = (.*)$", open(os.path.join(CSRC, "Makefile")).read(), re.M).group(1).split()
    assert HEADER in hdrs


def test_the_local_helpers_are_gone():
    for name, text in sources().items():
        for old in OLD_NAMES:
            assert not re.search(r"\b%s\b" % old, text), f"{old} in {name}"
    for name in os.listdir(CSRC):      # comments too: nothing points at a helper that no longer exists
        if os.path.isfile(os.path.join(CSRC, name)):
            text = open(os.path.join(CSRC, name), errors="replace").read()
            for old in OLD_NAMES:
                assert old not in text, f"{old} mentioned in {name}"


def test_the_hsum_tree_has_one_definition():
    """xor 4, then xor 1, then xor 2 of the same value: the 8-lane hsum of the reference"""
    tree = r"__shfl_xor\((\w+), 4\)[^}]{0,80}?__shfl_xor\(\1, 1\)[^}]{0,80}?__shfl_xor\(\1, 2\)"
    assert files_with(tree) == [HEADER]
    assert len(re.findall(tree, sources()[HEADER])) == 1


def test_the_softplus_gate_has_one_definition():
    assert files_with(r"\bsoftplus\b") == [HEADER]
    assert files_with(r"> 20\.0f \? \w+ : kr_logf\(") == [HEADER]
    assert len(re.findall(r"kr_logf\(1\.0f \+ kr_expf\(", sources()[HEADER])) == 1
    assert files_with(r"kr_logf\(1\.0f \+ kr_expf\(") == [HEADER]
