"""The "multi_mla_exact_split" option (docs/design/31-multi-mla-exact-split.md) without a GPU: both options are known in every layer, the refusal is a function
of its own asked last, the three kernels stand at the three sites that launch the one kernel and behind each function's own checks, the softmax all forms call is
one copy, no C-ABI symbol was added, and every instantiation of the new kernels is in the library."""
import os
import re
import subprocess

from tests.test_multi_pass_plan import case_passed

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "krasis_amd", "csrc")
OPT, MIN = "multi_mla_exact_split", "multi_mla_exact_split_min"
DOC = "31-multi-mla-exact-split.md"


def _src(name):
    return open(os.path.join(CSRC, name)).read()


def _body(src, head):
    body = src[src.index(head):]
    return body[:body.index("\n}\n")]


def _lib():
    from krasis_amd import _lib
    if not os.path.exists(_lib.lib_path()):
        subprocess.check_call(["make", "-C", CSRC])
    return _lib


def test_the_options_are_known_everywhere():
    from tests.util import option_field
    dec = _src("kr_decode.cpp")
    for o in (OPT, MIN):
        assert '!strcmp(name, "%s")' % o in dec and option_field(o) == o[len("multi_"):]
    assert "if (value < 1) return kr_fail(KR_ERR_VALUE" in dec[dec.index('"%s"))' % MIN):][:300]
    from krasis_amd.decode_store import CpuDecodeStore
    assert OPT in CpuDecodeStore.set_option.__doc__ and MIN in CpuDecodeStore.set_option.__doc__
    doc = open(os.path.join(ROOT, "docs", "design", DOC)).read()
    for word in (OPT, MIN, "kr_multi_mla_attn_kernel", "Not measured", "barrier", "kernel-resource-usage", "Bounds"):
        assert word in doc, word
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert OPT in readme and MIN in readme and "Not measured" in readme[readme.index(OPT):][:2500]
    assert "kr_multi_mla_split.hip" in _src("Makefile")
    assert os.path.exists(os.path.join(ROOT, "profiles", "multi_mla_exact_split.txt"))
    # the follow-up lines of the two documents that named this work are marked done; nothing was taken out of doc 30
    d30 = open(os.path.join(ROOT, "docs", "design", "30-multi-attn-exact-split.md")).read()
    assert "same three launches over latent rows. Not part of this change." in d30 and DOC in d30
    assert DOC in open(os.path.join(ROOT, "docs", "design", "15-multi-mla.md")).read()


def test_the_refusal_is_asked_last():
    from tests.util import FLAGS, recorded_refusal, rule_place_seen, rule_row
    pre = _src("kr_decode_prefill.cpp")
    assert pre.count("bool paged_refused(") == 1 and pre.count("for (const KrOptRule& r : kr_opt_rules)") == 1 and "(r.stand_back && back)) continue;" in pre      # one predicate, one walker: stands back where the entry point's paged refusal applies
    body = _body(_src("kr_decode_multi.cpp"), "int multi_refuse(kr_decode_store* s) {")
    order = [body.index(c) for c in ("kr_spec_pending_fail(s)", "kr_exact_refuse(s, true)", "return kr_option_rules(s, false);")]
    assert order == sorted(order)
    row = rule_row(OPT)      # "has none" and nothing else: no rival, no MLA step, no geometry rule, nothing to prepare; stands back
    assert row == '{"multi_mla_exact_split", &KrMultiOpts::mla_exact_split, ATTN_MLA, true, nullptr, nullptr, nullptr, 0, false, "", nullptr, nullptr, nullptr},'
    walk = pre[pre.index("int kr_option_rules("):]
    assert "graph_ok" not in walk[:walk.index("\n}\n")]
    # last of the options that existed then, ahead of "multi_extend_la_exact" alone: everything refused before is refused first, with its words
    assert FLAGS[-2:] == (OPT, "multi_extend_la_exact") and rule_place_seen(OPT) >= 8
    mine = 'RuntimeError: the "multi_mla_exact_split" option covers MLA layers only: this store has none (set the option to 0)'
    assert recorded_refusal("gqa/flat", OPT) == mine and recorded_refusal("gqa/flat", OPT, "multi_extend_la_exact") == mine
    assert recorded_refusal("la/flat", OPT, "multi_attn_exact_split") == recorded_refusal("la/flat", "multi_attn_exact_split")
    assert recorded_refusal("mla/flat", OPT) == "ok" and recorded_refusal("mla/paged", OPT) == "ok" and recorded_refusal("mla-3-heads/flat", OPT) == "ok"
    # the pass-level choice: the plan's (docs/design/32-multi-pass-plan.md)
    assert "o.opt = s->mopt;" in pre and "o.opt.mla_exact_split && has_mla && p.mla_pos + 1 >= o.opt.mla_exact_split_min" in _src("kr_multi_plan.h")
    assert case_passed("H") and "m.xs_split = pl.mla_xs_split;" in pre
    assert "int kr_option_rules(kr_decode_store* s, bool prepare);" in _src("kr_decode_internal.h")


def test_the_three_sites_take_the_split_behind_their_own_checks():
    multi = _src("kr_multi.hip")
    assert multi.count("kr_launch_multi_mla_split(") == 3      # kr_launch_multi_mla (flat and paged: one call behind KR_MMA_ALL), multi_mla_runs, kr_launch_multi_mla_xm
    sites = {"int kr_launch_multi_mla(const KrMultiMlaArgs& a_in, int B, hipStream_t st) {": ("kr_launch_multi_mla_split(a, B, st)", ("kr_multi_mla_ok(", "a.sc_ld % 32", "a.page_stride < 1", "kr_multi_mla_fd_ok(")),
             "static int multi_mla_runs(KrMultiMlaArgs& a, int B, hipStream_t st) {": ("kr_launch_multi_mla_split(a, a.mf_nruns, st)", ("kr_multi_mla_pf_args_ok(a)", "kr_multi_mla_fd_ok(", "!a.scores || a.sc_ld < 32")),
             "int kr_launch_multi_mla_xm(": ("kr_launch_multi_mla_split(a, n_runs, st)", ("kr_multi_mla_ok(", "a.sc_ld % 32", "a.page_stride < 1", "kr_multi_mla_xm_args_ok(a, x)", "kr_multi_mla_fd_ok("))}
    for fn, (site, checks) in sites.items():
        body = _body(multi, fn)
        assert body.count("kr_launch_multi_mla_split(") == 1 and site in body, fn
        first_launch = min(body.index("kr_launch_mla_absorb_mfma("), body.index("hipLaunchKernelGGL"))
        for c in checks:
            assert body.index(c) < first_launch < body.index(site), (fn, c)      # every check of the one-kernel path first, ahead of anything queued
        assert body.index("kr_multi_mla_prep_kernel") < body.index(site) < body.index("kr_launch_mla_wvc_mfma(")      # behind the prep launch, ahead of the w_vc projection
        assert "!a.fd_o && a.xs_split && kr_launch_multi_mla_split(" in body, fn      # the flash-decode pair takes the rows first: the flag is not read
    # multi_mla_runs is reached from kr_launch_multi_mla only, behind that function's checks
    outer = _body(multi, "int kr_launch_multi_mla(const KrMultiMlaArgs& a_in, int B, hipStream_t st) {")
    assert outer.index("a.page_stride < 1") < outer.index("if (a.mf_tiles) return multi_mla_runs(a, B, st);")
    hdr = _src("kr_multi.h")
    assert "int kr_launch_multi_mla_split(const KrMultiMlaArgs& a, int rows, hipStream_t st);" in hdr
    struct = re.search(r"struct KrMultiMlaArgs \{(.*?)\n\};", hdr, re.S).group(1)
    assert re.search(r"^\s*int xs_split;$", struct, re.M)


def test_the_softmax_is_one_copy_and_the_kernels_leave_the_runs_rows_first():
    split, multi = _src("kr_multi_mla_split.hip"), _src("kr_multi.hip")
    code = re.sub(r"//.*", "", split)
    assert '#include "kr_multi_softmax_dev.h"' in split and '#include "kr_mla_dev.h"' in split
    for src in (multi, split, _src("kr_multi_split.hip"), _src("kr_mla_dev.h")):
        assert "void kr_m_wave_softmax(" not in src
    assert _src("kr_multi_softmax_dev.h").count("void kr_m_wave_softmax(") == 1
    assert code.count("kr_m_wave_softmax(") == 1 and "asm" not in code and "extern __shared__" not in code      # static LDS only
    assert code.count("static_assert(") >= 3 and code.count("64 * 1024") >= 2
    assert code.count("if (kr_m_row_in_run(a, row)) return;") == 3      # all three leave the run kernels' rows
    for k in ("scores", "softmax", "pv"):      # ... ahead of the kernel's first barrier
        body = code[code.index("kr_multi_mla_split_%s_kernel(const KrMultiMlaArgs a) {" % k):]
        assert body.index("if (kr_m_row_in_run(a, row)) return;") < body.index("kr_m_wave_softmax(" if k == "softmax" else "__syncthreads()"), k
    scores = code[code.index("kr_multi_mla_split_scores_kernel(const KrMultiMlaArgs a) {"):code.index("kr_multi_mla_split_softmax_kernel(")]
    assert scores.index("if (t0 >= seq) return;") < scores.index("__syncthreads()")      # a tile past the row leaves ahead of every barrier too
    # the one kernel's statement sequence: the latent chain, its pair sum, the rope chain, its pair sum added, the scale
    seq = [scores.index(s) for s in ("acc = __builtin_fmaf(q4.x, kc[u], acc);", "float v = kr_mla_pair_hsum(acc, a2);", "acc = __builtin_fmaf(q4.x, kr[0], acc);",
                                     "v += kr_mla_pair_hsum(acc, a2);", "v *= a.sm_scale;")]
    assert seq == sorted(seq)
    one = re.sub(r"//.*", "", multi)
    one = one[one.index("kr_multi_mla_attn_kernel(const KrMultiMlaArgs a) {"):]
    for s in ("acc = __builtin_fmaf(qc[u], kc[u], acc);", "float v = kr_mla_pair_hsum(acc, a2);", "v += kr_mla_pair_hsum(acc, a2);", "v *= a.sm_scale;"):
        assert s in one, s


def test_library_exports_no_new_symbol_and_holds_the_new_kernels():
    _lib_mod = _lib()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib_mod.lib_path()], stdout=subprocess.PIPE, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if re.search(r" T kr_\w+$", line)}
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "krasis_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(kr_\w+)\s*\(", header))
    assert not exported - declared, sorted(exported - declared)
    assert not [n for n in exported if "split" in n and "multi" in n], exported
    names = subprocess.run(["nm", "-C", _lib_mod.lib_path()], stdout=subprocess.PIPE, text=True, check=True).stdout
    assert "kr_multi_mla_split_softmax_kernel" in names
    for nbc in (64, 32):
        for fp8 in ("true", "false"):
            for paged in ("true", "false"):
                for k in ("scores", "pv"):
                    assert "kr_multi_mla_split_%s_kernel<%s, %d, %s>" % (k, fp8, nbc, paged) in names, (k, fp8, nbc, paged)
