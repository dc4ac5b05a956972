"""The "multi_attn_exact_split" option (docs/design/30-multi-attn-exact-split.md) without a GPU: both options are known in every layer, the refusal is a function
of its own behind its siblings, the three kernels stand in every launcher that launches the one kernel, the softmax both forms call is one copy, no C-ABI symbol
was added, and every instantiation of the new kernels is in the library."""
import os
import re
import subprocess

from tests.test_multi_pass_plan import case_passed

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "krasis_amd", "csrc")
OPT, MIN = "multi_attn_exact_split", "multi_attn_exact_split_min"
DOC = "30-multi-attn-exact-split.md"


def _src(name):
    return open(os.path.join(CSRC, name)).read()


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
    for word in (OPT, MIN, "kr_multi_mla_attn_kernel", "Not measured", "barrier", "kernel-resource-usage"):
        assert word in doc, word
    assert OPT in open(os.path.join(ROOT, "README.md")).read()
    assert "kr_multi_split.hip" in _src("Makefile") and "kr_multi_softmax_dev.h" in _src("Makefile")
    assert os.path.exists(os.path.join(ROOT, "profiles", "multi_attn_exact_split.txt"))


def test_the_refusal_stands_behind_its_siblings():
    from tests.util import FLAGS, recorded_refusal, rule_place_seen, rule_row
    pre = _src("kr_decode_prefill.cpp")
    row = rule_row(OPT)      # "has none" and nothing else: no rival, no MLA step, no geometry rule, nothing to prepare; stands back
    assert row == '{"multi_attn_exact_split", &KrMultiOpts::attn_exact_split, ATTN_GQA, true, nullptr, nullptr, nullptr, 0, false, "", nullptr, nullptr, nullptr},'
    walk = pre[pre.index("int kr_option_rules("):]
    assert "graph_ok" not in walk[:walk.index("\n}\n")]
    assert pre.count("bool paged_refused(") == 1 and pre.count("for (const KrOptRule& r : kr_opt_rules)") == 1 and "(r.stand_back && back)) continue;" in pre      # one predicate, one walker: stands back where the entry point's paged refusal applies
    body = _src("kr_decode_multi.cpp")
    body = body[body.index("int multi_refuse("):body.index("int need_slots(")]
    assert body.index("kr_spec_pending_fail(s)") < body.index("kr_exact_refuse(s, true)") < body.index("return kr_option_rules(s, false);")
    assert FLAGS.index("multi_extend_exact_mfma") < FLAGS.index("multi_extend_mla_exact_mfma") < FLAGS.index(OPT)      # behind its siblings, as the recorded pairs show
    assert rule_place_seen(OPT) >= 8
    assert recorded_refusal("mla/flat", OPT) == 'RuntimeError: the "multi_attn_exact_split" option covers GQA layers only: this store has none (set the option to 0)'
    assert recorded_refusal("gqa/flat", OPT) == "ok" and recorded_refusal("hybrid/paged", OPT) == "ok" and recorded_refusal("gqa-3-per-kv/flat", OPT) == "ok"
    # the pass-level choice, by the longest attention of the per-row kernels: the plan's (docs/design/32-multi-pass-plan.md)
    assert "o.opt = s->mopt;" in pre and "p.attn_pos + 1 >= o.opt.attn_exact_split_min" in _src("kr_multi_plan.h")
    assert case_passed("H") and case_passed("B") and "m.xs_split = pl.xs_split;" in pre


def test_every_launcher_of_the_one_kernel_takes_the_split_and_the_softmax_is_one_copy():
    multi = _src("kr_multi.hip")
    assert multi.count("kr_launch_multi_gqa_split(") == 4      # flat and paged in kr_launch_multi_gqa, multi_gqa_runs, kr_launch_multi_gqa_xm
    for site in ("kr_launch_multi_gqa_split(a, B, st)", "kr_launch_multi_gqa_split(a, a.pf_nruns, st)", "kr_launch_multi_gqa_split(a, n_runs, st)"):
        assert site in multi, site
    for fn in ("int kr_launch_multi_gqa(", "static int multi_gqa_runs(const KrMultiGqaArgs& a, int B, size_t lds, hipStream_t st) {", "int kr_launch_multi_gqa_xm("):
        body = multi[multi.index(fn):]
        body = body[:body.index("\n}\n")]
        assert body.index("lds > KR_MULTI_GQA_LDS_MAX") < body.index("kr_launch_multi_gqa_split("), fn      # what the one kernel refuses is refused first
    split = _src("kr_multi_split.hip")
    code = re.sub(r"//.*", "", split)
    assert '#include "kr_multi_softmax_dev.h"' in split and '#include "kr_multi_softmax_dev.h"' in multi
    assert "void kr_m_wave_softmax(" not in multi and "void kr_m_wave_softmax(" not in split and _src("kr_multi_softmax_dev.h").count("void kr_m_wave_softmax(") == 1
    assert code.count("kr_m_wave_softmax(") == 1 and "asm" not in code
    assert code.count("if (kr_m_row_in_run(a, row)) return;") == 3      # all three leave the run kernels' rows
    for k in ("scores", "softmax", "pv"):      # ... ahead of the kernel's first barrier
        body = code[code.index("kr_multi_split_%s_kernel(const KrMultiGqaArgs a) {" % k):]
        assert body.index("if (kr_m_row_in_run(a, row)) return;") < body.index("kr_m_wave_softmax(" if k == "softmax" else "__syncthreads()"), k


def test_library_exports_no_new_symbol_and_holds_the_new_kernels():
    _lib_mod = _lib()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib_mod.lib_path()], stdout=subprocess.PIPE, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if re.search(r" T kr_\w+$", line)}
    assert not [n for n in exported if "split" in n and "multi" in n], exported
    names = subprocess.run(["nm", "-C", _lib_mod.lib_path()], stdout=subprocess.PIPE, text=True, check=True).stdout
    assert "kr_multi_split_softmax_kernel" in names
    for nb in (8, 16, 32):
        for fp8 in ("true", "false"):
            for paged in ("true", "false"):
                for k in ("scores", "pv"):
                    assert "kr_multi_split_%s_kernel<%d, %s, %s>" % (k, nb, fp8, paged) in names, (k, nb, fp8, paged)
