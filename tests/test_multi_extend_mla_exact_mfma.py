"""The "multi_extend_mla_exact_mfma" option (docs/design/29-multi-extend-mla-exact-mfma.md) without a GPU: the option is known in every layer, the refusal is a
rule of the ordered rule list behind the GQA option's, the new launcher checks before it launches and ends with the w_vc projection, no C-ABI symbol was added, and the new
kernels are in the library.  (The option adds no host-only helper: its tile tables are kr_pf_tiles.h / kr_xm_tiles.h at the widths 64 / nh and 32 / nh, which
tests/xm_tiles_check.cpp checks for every width from 1 to 64.)"""
import os
import re
import subprocess

from tests.test_multi_pass_plan import case_passed

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "krasis_amd", "csrc")
OPT = "multi_extend_mla_exact_mfma"
DOC = "29-multi-extend-mla-exact-mfma.md"


def _src(name):
    return open(os.path.join(CSRC, name)).read()


def _lib():
    from krasis_amd import _lib
    if not os.path.exists(_lib.lib_path()):
        subprocess.check_call(["make", "-C", CSRC])
    return _lib


def _body(text, head):
    body = text[text.index(head):]
    return body[:body.index("\n}\n")]


def test_the_option_is_known_everywhere():
    assert '!strcmp(name, "%s")' % OPT in _src("kr_decode.cpp")
    from tests.util import option_field
    assert option_field(OPT) == "extend_mla_exact_mfma"
    header = open(os.path.join(ROOT, "include", "krasis_hip.h")).read()
    assert '"%s"' % OPT in header and DOC in header
    from krasis_amd.decode_store import CpuDecodeStore
    for fn in (CpuDecodeStore.set_option, CpuDecodeStore.extend_multi, CpuDecodeStore.prefill_slot):
        assert OPT in fn.__doc__, fn.__name__
        said = fn.__doc__[fn.__doc__.index(OPT):]
        assert '"multi_mla_fast"' in said and "exact bits" in said, fn.__name__      # what a mixed pass gives under "multi_mla_fast"
    doc = open(os.path.join(ROOT, "docs", "design", DOC)).read()
    for section in ("Contract", "Kernels", "Resources", "Bounds", "Measured", "Out of scope"):
        assert "## " + section in doc, section
    assert OPT in doc
    assert OPT in open(os.path.join(ROOT, "README.md")).read()
    assert OPT in open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "kr_multi_mla_xm.hip" in _src("Makefile") and "kr_xm_mla_dev.h" in _src("Makefile")
    prof = open(os.path.join(ROOT, "profiles", "multi_extend_mla_exact_mfma.txt")).read()
    assert "kernel-resource-usage" in prof and "kr_multi_mla_xm_scores_kernel" in prof and "kr_multi_mla_xm_pv512_kernel" in prof


def test_the_refusal_is_a_function_of_its_own_behind_every_earlier_clause():
    from tests.util import recorded_refusal, rule_place_seen, rule_row
    pre = _src("kr_decode_prefill.cpp")
    span = pre[pre.index("int kr_exact_refuse("):pre.index("int kr_spec_refuse(")]
    assert OPT not in span and "multi_extend" not in span                     # kr_exact_refuse holds the base clauses only
    assert OPT not in rule_row("multi_extend_exact_mfma")                     # and the GQA option's rule knows nothing of this one
    row = rule_row(OPT)
    assert row.startswith('{"multi_extend_mla_exact_mfma", &KrMultiOpts::extend_mla_exact_mfma, ATTN_MLA, true, "multi_extend_mla_flash", &KrMultiOpts::extend_mla_flash, "the runs of >= 2 tokens of the MLA layers", 0, false, "",')
    assert re.search(r"KR_ERR_VALUE[^;]*divide 32", row) and "kr_mla_exact_mfma_ok(L.nh, L.klr, L.rd)" in row and row.rstrip().endswith("nullptr, nullptr},")      # the prompt pass's own geometry rule; nothing to prepare
    assert pre.count("bool paged_refused(") == 1 and pre.count("for (const KrOptRule& r : kr_opt_rules)") == 1 and "(r.stand_back && back)) continue;" in pre      # one predicate, one walker: stands back where the entry point's paged refusal applies
    body = _src("kr_decode_multi.cpp")
    body = body[body.index("int multi_refuse("):body.index("int need_slots(")]
    assert body.index("kr_spec_pending_fail(s)") < body.index("kr_exact_refuse(s, true)") < body.index("return kr_option_rules(s, false);")
    # as a caller sees it: both run options -- the message names both; every message names the option; behind the GQA option's rule
    assert rule_place_seen(OPT) >= 8
    assert recorded_refusal("mla/flat", OPT, "multi_extend_mla_flash") == 'RuntimeError: the "multi_extend_mla_exact_mfma" and "multi_extend_mla_flash" options both claim the runs of >= 2 tokens of the MLA layers: set one of them to 0'
    assert recorded_refusal("la/flat", OPT) == 'RuntimeError: the "multi_extend_mla_exact_mfma" option covers MLA layers only: this store has none (set the option to 0)'
    assert recorded_refusal("la/flat", OPT, "multi_extend_exact_mfma") == recorded_refusal("la/flat", "multi_extend_exact_mfma")
    assert recorded_refusal("mla-3-heads/flat", OPT).startswith("ValueError: multi_extend_mla_exact_mfma: MLA geometry heads 3 kv_lora_rank 256 rope 64 not covered (the head count must divide 32")
    assert recorded_refusal("mla/flat", OPT) == "ok" and recorded_refusal("mla/paged", OPT) == "ok"


def test_the_scores_body_is_a_header_of_its_own():
    dev = _src("kr_xm_mla_dev.h")
    assert re.search(r"template <bool FP8, bool ROPE, bool PAGED, class Rows>\s*__device__ __forceinline__ void kr_xm_mla_scores_body\(", dev)
    assert dev.count("__builtin_amdgcn_mfma_f32_32x32x2f32") == 1 and "kr_xm_cache_row<PAGED>(" in dev and "__shared__" not in dev
    code = re.sub(r"//.*", "", dev)
    assert code.index("if (p_lo > p_max) return;") < code.index("__syncthreads()")      # the exit stays ahead of every barrier
    assert code.index("kr_xm_cache_row<PAGED>(") < code.index("for (int k0 = 0; k0 < K; k0 += 64)")      # the page is looked up once, ahead of the k loop
    multi = _src("kr_multi_mla_xm.hip")
    assert "kr_xm_mla_scores_body<FP8, ROPE, PAGED>(" in multi and "kr_xm_pv_body<FP8, 512, 32, PAGED>(" in multi
    assert "kr_m_run_row(i, off, cnt, t)" in multi and "extern __shared__" not in re.sub(r"//.*", "", multi)      # the pass's flatten; static LDS only
    assert "kr_launch_multi_xm_softmax(g, x, B, st)" in multi and "kr_launch_multi_xm_pv(g, x, st)" in multi      # passes B and C (256) are the GQA option's kernels


def test_the_launcher_and_the_pass():
    hdr = _src("kr_multi.h")
    body = re.search(r"struct KrMultiMlaArgs \{(.*?)\n\};", hdr, re.S).group(1)
    assert body.rstrip().endswith("const int* mf_runs; const int* mf_tiles; int mf_nruns, mf_ntiles, mf_units;")      # the struct did not grow
    assert "struct KrMultiXmArgs { const int* tiles_a; const int* tiles_c; int n_a, n_c; float* inv; float* tmax; int kv_end; };" in hdr
    multi = _src("kr_multi.hip")
    assert multi.index("int kr_launch_multi_mla(const KrMultiMlaArgs& a_in, int B, hipStream_t st) {") < multi.index("int kr_launch_multi_mla_xm(")
    mine = _body(multi, "int kr_launch_multi_mla_xm(")
    assert "a.mf_runs = runs; a.mf_nruns = n_runs; a.mf_units = units; a.mf_tiles = nullptr;" in mine
    first_launch = min(mine.index("kr_launch_mla_absorb_mfma("), mine.index("kr_multi_mla_prep_kernel"))
    for check in ("kr_multi_mla_ok(", "kr_multi_mla_xm_args_ok(a, x)", "kr_multi_mla_fd_ok("):
        assert mine.index(check) < first_launch, check                        # every check ahead of the first launch: a layer fails whole
    order = [mine.index(s) for s in ("kr_launch_mla_absorb_mfma(", "hipLaunchKernelGGL((kr_multi_mla_prep_kernel", "kr_launch_multi_mla_fd(a, n_runs, st)",
                                     "kr_launch_multi_mla_xm_attn(a, x, B, st)", "kr_launch_mla_wvc_mfma(")]
    assert order == sorted(order)
    assert "(a.nh + KR_MM_HG - 1) / KR_MM_HG, n_runs)" in mine                # the per-row kernel over the first n_runs rows
    assert mine.rstrip().endswith("kr_launch_mla_wvc(m, st, B);\n    return 0;")      # ends with the w_vc projection over all rows
    pre = _src("kr_decode_prefill.cpp")
    assert "o.opt = s->mopt;" in pre and "o.opt.extend_mla_exact_mfma ? KR_MP_RUNS_XM" in _src("kr_multi_plan.h") and case_passed("F") and case_passed("K")      # never in a verify pass (docs/design/32-multi-pass-plan.md)
    assert case_passed("J")                                                   # the tables at 64 / nh and 32 / nh, shared with a GQA layer of the same group size
    assert "kr_launch_multi_mla_xm(m, multi_xm_args(P, L.nh, 1), P.runs, P.nruns, P.plan.n_unit, Cc, st)" in pre


def test_library_exports_exactly_the_declared_symbols_and_holds_the_new_kernels():
    _lib_mod = _lib()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib_mod.lib_path()], stdout=subprocess.PIPE, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if re.search(r" T kr_\w+$", line)}
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "krasis_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(kr_\w+)\s*\(", header))
    assert not exported - declared, sorted(exported - declared)
    assert set(_lib_mod.SYMBOLS) <= exported
    assert not [n for n in exported if "_xm" in n or "exact_mfma" in n or "mla_pf" in n or "mla_flash" in n]
    names = subprocess.run(["nm", "-C", _lib_mod.lib_path()], stdout=subprocess.PIPE, text=True, check=True).stdout
    for fp8 in ("true", "false"):
        for paged in ("true", "false"):
            for rope in ("true", "false"):
                k = "kr_multi_mla_xm_scores_kernel<%s, %s, %s>" % (fp8, rope, paged)
                assert k in names, k
            k = "kr_multi_mla_xm_pv512_kernel<%s, %s>" % (fp8, paged)
            assert k in names, k
