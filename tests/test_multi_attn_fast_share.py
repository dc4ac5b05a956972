"""The item list of "multi_attn_fast_paged" = 2 (docs/design/44-multi-attn-fast-share.md) without a GPU: krasis_amd/csrc/kr_fd_share.h is host-only, and
tests/fd_share_check.cpp drives it on hand-made tables -- as built, and under the address and undefined-behaviour sanitizers, each a program of its own."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "krasis_amd", "csrc")


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]],
                         ids=["plain", "sanitizers"])
def test_item_list_program(tmp_path, flags):
    """equal page ids give a group, a differing id in the middle of a chunk or a chunk that is not full gives none, groups are cut at R in batch order, R < 2
    gives no list, rows of a run are skipped, and every live (row, chunk) pair lies in exactly one item"""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "fd_share_check")
    subprocess.check_call([cxx, "-std=c++17", "-Wall", "-Werror", *flags, "-I", CSRC, "-o", exe, os.path.join(ROOT, "tests", "fd_share_check.cpp")])
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert run.returncode == 0 and "fd share ok" in run.stdout, run.stdout
