"""The batched pass's plan (krasis_amd/csrc/kr_multi_plan.h, docs/design/32-multi-pass-plan.md) without a GPU: the header is host only, the pass calls it once
and keeps allocation, upload and launch, the slots' state has one table buffer, Chunk has one batched-pass member, and the planner passes its stand-alone check --
hand-written cases A .. J and the properties K -- under AddressSanitizer and UBSan in a child process.  plan_check() is what the option tests share: the program
is compiled and run once per session."""
import functools
import os
import re
import shutil
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "krasis_amd", "csrc")
CHECK = os.path.join(ROOT, "tests", "multi_plan_check.cpp")


def _src(name):
    return open(os.path.join(CSRC, name)).read()


@functools.lru_cache(maxsize=None)
def plan_check():
    """(source text of tests/multi_plan_check.cpp, its output): compiled alone with -fsanitize=address,undefined and run as a child process (nothing sanitized is
    loaded into Python); asserts that it passed"""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "multi_plan_check")
        subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                               "-I", CSRC, "-o", exe, CHECK])      # runtimes inside the program: no library order to get wrong
        run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert run.returncode == 0 and "multi plan ok" in run.stdout, run.stdout
    return open(CHECK).read(), run.stdout


def case_passed(letter):
    """the check program holds the case's marker and the case ran to its end"""
    src, out = plan_check()
    return "// case %s: " % letter in src and "case %s ok" % letter in out


def test_the_plan_program_under_sanitizers():
    for letter in "ABCDEFGHIJK":
        assert case_passed(letter), letter


def test_the_planner_is_host_only():
    src = _src("kr_multi_plan.h")
    code = re.sub(r"//.*", "", src)
    assert "hip" not in code.lower() and "__device__" not in code
    assert set(re.findall(r"#include [<\"]([^>\"]+)[>\"]", src)) == {"stddef.h", "stdint.h", "vector", "kr_lc_tiles.h", "kr_mf_tiles.h", "kr_pf_tiles.h", "kr_xm_tiles.h"}
    assert "kr_multi_plan.h" in _src("Makefile")
    pre = _src("kr_decode_prefill.cpp")
    assert '#include "kr_multi_plan.h"' in pre
    for tiles in ("kr_pf_tiles.h", "kr_xm_tiles.h", "kr_lc_tiles.h", "kr_mf_tiles.h"):
        assert '#include "%s"' % tiles not in pre, tiles      # through the plan only
    assert code.count("kr_pf_build_tiles(") == 1 and code.count("kr_mf_build_tiles(") == 1 and code.count("kr_lc_build(") == 1      # one call site per builder
    assert code.count("r.counts[i] >= 2") == 1      # the run scan is written once


def test_the_pass_keeps_allocation_upload_and_launch():
    pre = _src("kr_decode_prefill.cpp")
    p = pre[pre.index("int kr_multi_pass("):]
    order = [p.index(w) for w in ("pf_layout(s, (size_t)n, true, true, st, Lo)", "KrMultiPlanOpts o{};", "kr_multi_plan(o, ", "M.fd_ready = true;", "M.mla_fd_ready = true;",
                                  "M.fd_o.ensure(plan.fd_o_bytes)", "M.scratch.ensure(Lo.total)", "M.tiles.ensure(", "hipMemcpyAsync(M.tiles.p, plan.tables.data()",
                                  "run_layer(s, cx, l)", "final_rows(s, cx, (float*)M.logits.p)")]
    assert order == sorted(order)
    assert p.count("hipMemcpyAsync(") == 1 and "if (!plan.tables.empty())" in p      # one upload of the tables, when there are any
    assert p.count("kr_pf_build_tiles") == 0 and p.count("h_counts[") == 0           # no decision left in the pass
    for text in ('"multi_attn_fast: position %d needs %d chunks of %d positions (at most 1024)", plan.attn_pos, plan.fd_chunks, plan.fd_chunk',
                 '"multi_mla_fast: position %d needs %d chunks of %d positions (at most 1024)", plan.mla_pos, plan.mla_chunks, plan.mla_chunk'):
        assert text in p, text
    assert p.index("case KR_MP_GQA_CHUNKS") < p.index("case KR_MP_MLA_CHUNKS")
    state = _src("kr_decode_internal.h")
    assert "DevBuf tiles;" in state
    for gone in ("pf_tiles", "xm_tiles", "mf_tiles", "lc_tiles"):
        assert not re.search(r"DevBuf[^;]*\b%s\b" % gone, state), gone
    assert "DevBuf lc_scratch;" in state and "DevBuf xm_rows;" in state


def test_chunk_has_one_batched_pass_member_and_three_arg_functions():
    pre = _src("kr_decode_prefill.cpp")
    chunk = re.search(r"\nstruct Chunk \{(.*?)\n\};", pre, re.S).group(1)
    assert "const MultiPass* mp = nullptr;" in chunk and not re.search(r"\bm_\w+", chunk)
    assert "m_slots" not in pre and "cx.m_" not in pre
    for fn in ("static KrMultiLaArgs multi_la_args(", "static KrMultiGqaArgs multi_gqa_args(", "static KrMultiMlaArgs multi_mla_args("):
        assert pre.count(fn) == 1 and pre.index(fn) < pre.index("static int run_layer("), fn
    layer = pre[pre.index("static int run_layer("):pre.index("static void run_final(")]
    assert layer.count("if (cx.mp) {") == 3 and "KrMultiGqaArgs m{}" not in layer and "KrMultiMlaArgs m{}" not in layer and "KrMultiLaArgs m{}" not in layer


def test_the_refusals_share_one_predicate_and_one_loop():
    pre = _src("kr_decode_prefill.cpp")
    assert pre.count("pg.paged() && s->opt_multi_attn_fast && !s->opt_multi_attn_fast_paged") == 1      # the predicate's one copy ...
    assert "bool paged_refused(const kr_decode_store* s) { return s->multi && s->multi->pg.paged() && s->opt_multi_attn_fast && !s->opt_multi_attn_fast_paged; }" in pre
    assert "pg.paged() && s->opt_multi_attn_fast" not in _src("kr_decode_multi.cpp")
    for fn in ("int kr_xm_refuse(", "int kr_mla_xm_refuse(", "int kr_xs_refuse(", "int kr_mla_xs_refuse("):
        body = pre[pre.index(fn):]
        body = body[:body.index("\n}\n")]
        assert "|| paged_refused(s)) return KR_OK;" in body and body.count("has_attn(s, ATTN_") == 1, fn
    exact = pre[pre.index("int kr_exact_refuse("):pre.index("int kr_spec_refuse(")]
    assert exact.count("!paged_refused(s)") == 3 and exact.count("has_attn(s, ATTN_") == 4
    refuse = re.search(r"int paged_refuse\(kr_decode_store\* s\) \{(.*?)\n\}", _src("kr_decode_multi.cpp"), re.S).group(1)
    assert "if (paged_refused(s))" in refuse
    hdr = _src("kr_decode_internal.h")
    assert "bool paged_refused(const kr_decode_store* s);" in hdr and "bool has_attn(const kr_decode_store* s, int kind);" in hdr
    order = [pre.index(f) for f in ("int kr_exact_refuse(", "int kr_xm_refuse(", "int kr_mla_xm_refuse(", "int kr_xs_refuse(", "int kr_mla_xs_refuse(")]
    assert order == sorted(order)      # five functions, in the order multi_refuse asks them
