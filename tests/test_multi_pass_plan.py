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
    assert set(re.findall(r"#include [<\"]([^>\"]+)[>\"]", src)) == {"stddef.h", "stdint.h", "vector", "kr_lc_tiles.h", "kr_mf_tiles.h", "kr_multi_opts.h", "kr_pf_tiles.h", "kr_xm_tiles.h"}
    opts = _src("kr_multi_opts.h")      # the options value the plan is handed whole: host only, nothing included
    assert "hip" not in re.sub(r"//.*", "", opts).lower() and "#include" not in opts and "kr_multi_opts.h" in _src("Makefile")
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
    from tests.util import FLAGS, recorded_refusal
    pre = _src("kr_decode_prefill.cpp")
    assert pre.count("pg.paged() && s->mopt.attn_fast && !s->mopt.attn_fast_paged") == 1      # the predicate's one copy ...
    assert "bool paged_refused(const kr_decode_store* s) { return s->multi && s->multi->pg.paged() && s->mopt.attn_fast && !s->mopt.attn_fast_paged; }" in pre
    assert pre.count("bool paged_refused(") == 1 and "pg.paged() && s->mopt.attn_fast" not in _src("kr_decode_multi.cpp")
    # ... asked once, by the one walker of the one rule list: nine rules, in the order a caller sees (tests/test_multi_option_refusals_gpu.py)
    assert pre.count("paged_refused(s)") == 1 and pre.count("for (const KrOptRule& r : kr_opt_rules)") == 1 and pre.count("kr_opt_rules") == 2
    walk = pre[pre.index("int kr_option_rules("):]
    walk = walk[:walk.index("\n}\n")]
    assert "const bool back = paged_refused(s);" in walk and "(r.stand_back && back)) continue;" in walk and walk.count("has_attn(s, r.kind)") == 1
    table = pre[pre.index("static const KrOptRule kr_opt_rules[] = {"):pre.index("int kr_option_rules(")]
    assert re.findall(r'\n    \{"(multi_\w+)", &KrMultiOpts::(\w+), ATTN_\w+, (true|false),', table) == [(f, f[len("multi_"):], "false" if f == "multi_mla_fast" else "true") for f in FLAGS[2:]]
    exact = pre[pre.index("int kr_exact_refuse("):pre.index("int kr_spec_refuse(")]
    assert "paged_refused" not in exact and "has_attn" not in exact and "hipSetDevice" not in exact and "_prepare(" not in exact      # base clauses only, and no work
    refuse = re.search(r"int paged_refuse\(kr_decode_store\* s\) \{(.*?)\n\}", _src("kr_decode_multi.cpp"), re.S).group(1)
    assert "if (paged_refused(s))" in refuse
    hdr = _src("kr_decode_internal.h")
    assert "bool paged_refused(const kr_decode_store* s);" in hdr and "bool has_attn(const kr_decode_store* s, int kind);" in hdr
    assert "int kr_option_rules(kr_decode_store* s, bool prepare);" in hdr and not re.search(r"int kr_\w+_refuse\((?!kr_decode_store\* s(, bool slots)?\);)", hdr)
    assert len(re.findall(r"\nint kr_\w*refuse\(", pre)) == 2      # kr_exact_refuse and kr_spec_refuse: the five option functions are gone
    # what standing back gives a caller: on paged slots under "multi_attn_fast" alone the entry point's words come back whatever else is set, except that
    # "multi_mla_fast" does not stand back
    for store in ("la/paged", "gqa/paged", "hybrid/paged"):
        for f in FLAGS[3:]:
            assert recorded_refusal(store, "multi_attn_fast", f).startswith('RuntimeError: "multi_attn_fast" does not read paged slots'), (store, f)
        assert 'the "multi_mla_fast" option covers MLA layers only: this store has none' in recorded_refusal(store, "multi_attn_fast", "multi_mla_fast")


def test_preparing_is_not_refusing():
    """the LDS windows are raised by the walk's second visit, which multi_begin makes once every refusal has passed; the refusing visit does no work"""
    pre, multi = _src("kr_decode_prefill.cpp"), _src("kr_decode_multi.cpp")
    walk = pre[pre.index("int kr_option_rules("):]
    walk = walk[:walk.index("\n}\n")]
    prep = walk[walk.index("if (prepare) {"):walk.index("const char* kind")]
    assert "hipSetDevice" in prep and "r.prepare(s)" in prep and prep.rstrip().endswith("continue;\n        }") and "hipSetDevice" not in walk.replace(prep, "")
    begin = multi[multi.index("int multi_begin("):multi.index("int slot_in_range(")]
    assert begin.index("if (int rc = multi_refuse(s)) return rc;") < begin.index("return kr_option_rules(s, true);")
    refuse = multi[multi.index("int multi_refuse("):multi.index("int need_slots(")]
    order = [refuse.index(w) for w in ("kr_spec_pending_fail(s)", "kr_exact_refuse(s, true)", "return kr_option_rules(s, false);")]
    assert order == sorted(order) and refuse.count("return") == 3
    p = pre[pre.index("int kr_multi_pass("):]
    assert "kr_option_rules" not in p and "pf_prepare" not in p and "lc_prepare" not in p      # never inside the pass
