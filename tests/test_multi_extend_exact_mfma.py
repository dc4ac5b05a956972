"""The "multi_extend_exact_mfma" option (docs/design/28-multi-extend-exact-mfma.md) without a GPU: the option is known in every layer, the single-sequence exact
prompt pass and the batched runs share one body per matrix-core pass, the refusal is a function of its own behind kr_exact_refuse, no C-ABI symbol was added, the
new kernels are in the library, and the tile tables -- a host-only header -- pass their stand-alone check under AddressSanitizer and UBSan in a child process."""
import os
import re
import shutil
import subprocess

from tests.test_multi_pass_plan import case_passed

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "krasis_amd", "csrc")
OPT = "multi_extend_exact_mfma"
DOC = "28-multi-extend-exact-mfma.md"


def _src(name):
    return open(os.path.join(CSRC, name)).read()


def _lib():
    from krasis_amd import _lib
    if not os.path.exists(_lib.lib_path()):
        subprocess.check_call(["make", "-C", CSRC])
    return _lib


def test_the_option_is_known_everywhere():
    assert '!strcmp(name, "%s")' % OPT in _src("kr_decode.cpp")
    from tests.util import option_field
    assert option_field(OPT) == "extend_exact_mfma"
    header = open(os.path.join(ROOT, "include", "krasis_hip.h")).read()
    assert '"%s"' % OPT in header and DOC in header
    from krasis_amd.decode_store import CpuDecodeStore
    for fn in (CpuDecodeStore.set_option, CpuDecodeStore.extend_multi, CpuDecodeStore.prefill_slot):
        assert OPT in fn.__doc__, fn.__name__
    for fn in (CpuDecodeStore.set_option, CpuDecodeStore.extend_multi):
        assert "unit rows" in fn.__doc__ and "exact bits" in fn.__doc__, fn.__name__      # what a mixed pass gives under "multi_attn_fast"
    doc = open(os.path.join(ROOT, "docs", "design", DOC)).read()
    assert OPT in doc and "Out of scope" in doc
    assert OPT in open(os.path.join(ROOT, "README.md")).read()
    assert OPT in open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "kr_multi_xm.hip" in _src("Makefile") and "kr_xm_dev.h" in _src("Makefile") and "kr_xm_tiles.h" in _src("Makefile")


def test_the_refusal_is_a_function_of_its_own_behind_every_earlier_clause():
    from tests.util import recorded_refusal, rule_place_seen, rule_row
    pre = _src("kr_decode_prefill.cpp")
    span = pre[pre.index("int kr_exact_refuse("):pre.index("int kr_spec_refuse(")]
    assert OPT not in span and "multi_extend" not in span                     # kr_exact_refuse holds the base clauses only
    row = rule_row(OPT)
    assert row.startswith('{"multi_extend_exact_mfma", &KrMultiOpts::extend_exact_mfma, ATTN_GQA, true, "multi_extend_flash", &KrMultiOpts::extend_flash, "the runs of >= 2 tokens of the GQA layers", 0, false, "",')
    assert re.search(r"KR_ERR_VALUE[^;]*not covered", row) and "kr_pfm_gqa_exact_mfma_ok(g)" in row and row.rstrip().endswith("nullptr, nullptr},")      # the prompt pass's own geometry rule; nothing to prepare
    assert pre.count("bool paged_refused(") == 1 and pre.count("for (const KrOptRule& r : kr_opt_rules)") == 1 and "(r.stand_back && back)) continue;" in pre      # one predicate, one walker: stands back where the entry point's paged refusal applies
    body = _src("kr_decode_multi.cpp")
    body = body[body.index("int multi_refuse("):body.index("int need_slots(")]
    assert body.index("kr_spec_pending_fail(s)") < body.index("kr_exact_refuse(s, true)") < body.index("return kr_option_rules(s, false);")
    # as a caller sees it: both run options -- the message names both, ahead of "has none" and only once the rival's own rule has passed; every message names the option
    assert rule_place_seen(OPT) >= 8
    assert recorded_refusal("gqa/flat", OPT, "multi_extend_flash") == 'RuntimeError: the "multi_extend_exact_mfma" and "multi_extend_flash" options both claim the runs of >= 2 tokens of the GQA layers: set one of them to 0'
    assert recorded_refusal("la/flat", OPT, "multi_extend_flash") == recorded_refusal("la/flat", "multi_extend_flash")
    assert recorded_refusal("la/flat", OPT) == 'RuntimeError: the "multi_extend_exact_mfma" option covers GQA layers only: this store has none (set the option to 0)'
    assert recorded_refusal("gqa-3-per-kv/flat", OPT).startswith("ValueError: multi_extend_exact_mfma: GQA geometry nh 6 nkv 2 head_dim 64 not covered (heads per KV head must divide 32")
    assert recorded_refusal("gqa/flat", OPT) == "ok" and recorded_refusal("hybrid/paged", OPT) == "ok"


def test_one_body_two_callers():
    dev = _src("kr_xm_dev.h")
    assert re.search(r"template <bool FP8, bool PAGED, class Rows>\s*__device__ __forceinline__ void kr_xm_scores_body\(", dev)
    assert re.search(r"template <bool FP8, int HD, int PS, bool PAGED, class Rows>[^\n]*\s*__device__ __forceinline__ void kr_xm_pv_body\(", dev)
    assert dev.count("__builtin_amdgcn_mfma_f32_32x32x2f32") == 2 and "max(ptab[p >> psh], 0)" in dev
    assert "asm" not in re.sub(r"//.*", "", dev) and "__shared__" not in dev
    single = _src("kr_attn_exact_mfma.hip")
    assert "kr_xm_scores_body<FP8, false>(" in single and "kr_xm_pv_body<FP8, HD, PS, false>(" in single and single.count("KrXmRowsIdentity()") == 2
    gqa = single[:single.index("kr_mla_scores_mfma_kernel")]
    assert "__builtin_amdgcn_mfma_f32_32x32x2f32" not in gqa                  # the GQA bodies moved whole; the MLA scores kernel is text of its own, untouched
    for word in ("slot", "page_table", "pf_runs"):
        assert not re.search(r"\b%s" % word, re.sub(r"//.*", "", single)), word
    multi = _src("kr_multi_xm.hip")
    code = re.sub(r"//.*", "", multi)
    assert "kr_xm_scores_body<FP8, PAGED>(" in multi and "kr_xm_pv_body<FP8, HD, 64, PAGED>(" in multi
    assert "kr_m_run_row(i, off, cnt, t)" in multi and "a.page_table + (size_t)slot * a.page_stride" in multi
    assert "__builtin_amdgcn_mfma" not in code and "asm" not in code and "extern __shared__" not in code      # no matrix-core text of its own, static LDS only
    for hd in (64, 128, 256):
        assert "KR_XC(true, %d)" % hd in multi and "KR_XC(false, %d)" % hd in multi
    # the resource table: parent against this commit, every existing instantiation unchanged
    prof = open(os.path.join(ROOT, "profiles", "multi_extend_exact_mfma.txt")).read()
    assert "kernel-resource-usage" in prof and "kr_mla_scores_mfma_kernel" in prof and "kr_pfm_gqa_pv_mfma_kernel<true, 512, 32>" in prof


def test_the_launcher_and_the_pass():
    hdr = _src("kr_multi.h")
    body = re.search(r"struct KrMultiGqaArgs \{(.*?)\n\};", hdr, re.S).group(1)
    assert body.rstrip().endswith("const int* pf_runs; const int* pf_tiles; int pf_nruns, pf_ntiles, pf_units;")      # the struct did not grow
    assert "struct KrMultiXmArgs { const int* tiles_a; const int* tiles_c; int n_a, n_c; float* inv; float* tmax; int kv_end; };" in hdr
    multi = _src("kr_multi.hip")
    assert multi.index("static int multi_gqa_runs(const KrMultiGqaArgs& a, int B, size_t lds, hipStream_t st) {") < multi.index("int kr_launch_multi_gqa_xm(")
    mine = multi[multi.index("int kr_launch_multi_gqa_xm("):]
    mine = mine[:mine.index("\n}\n")]
    assert "a.pf_runs = runs; a.pf_nruns = n_runs; a.pf_units = units; a.pf_tiles = nullptr;" in mine
    assert mine.index("kr_multi_xm_args_ok(a, x)") < mine.index("kr_multi_gqa_prep_kernel") and mine.index("lds > KR_MULTI_GQA_LDS_MAX") < mine.index("kr_multi_gqa_prep_kernel")
    assert "dim3(a.nh + a.nkv, B)" in mine and "dim3(a.nkv, n_runs)" in mine and "kr_launch_multi_fd(a, n_runs, a.fd_chunks, st)" in mine
    assert mine.rstrip().endswith("return kr_launch_multi_xm(a, x, B, st);")
    pre = _src("kr_decode_prefill.cpp")
    plan = _src("kr_multi_plan.h")      # the pass's decisions are the plan's (docs/design/32-multi-pass-plan.md): its check program's cases stand for the lines once pinned here
    assert "o.opt = s->mopt;" in pre and "o.opt.extend_exact_mfma ? KR_MP_RUNS_XM" in _src("kr_multi_plan.h") and case_passed("F")      # never in a verify pass
    assert "plan.need_scores && M.scores.ensure(plan.score_bytes)" in pre and case_passed("A") and "(has_mla && !mla_flash && p.mla_row_attn)" in plan and case_passed("D")
    assert case_passed("E") and case_passed("K")                              # the row stride: a multiple of 64 under the option, of 32 otherwise
    tiles = re.sub(r"//.*", "", _src("kr_xm_tiles.h"))
    assert "hip" not in tiles.lower() and "__device__" not in tiles


def test_library_exports_exactly_the_declared_symbols_and_holds_the_new_kernels():
    _lib_mod = _lib()
    out = subprocess.run(["nm", "-D", "--defined-only", _lib_mod.lib_path()], stdout=subprocess.PIPE, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if re.search(r" T kr_\w+$", line)}
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "krasis_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(kr_\w+)\s*\(", header))
    assert not exported - declared, sorted(exported - declared)
    assert set(_lib_mod.SYMBOLS) <= exported
    assert not [n for n in exported if "_xm" in n or "exact_mfma" in n]
    names = subprocess.run(["nm", "-C", _lib_mod.lib_path()], stdout=subprocess.PIPE, text=True, check=True).stdout
    for k in ("kr_multi_xm_softmax_kernel", "kr_multi_xm_scores_kernel<true, true>", "kr_multi_xm_scores_kernel<false, false>",
              "kr_multi_xm_pv_kernel<true, 256, true>", "kr_multi_xm_pv_kernel<false, 128, false>", "kr_multi_xm_pv_kernel<false, 64, true>"):
        assert k in names, k


def test_tile_table_program_under_sanitizers(tmp_path):
    """tiles cover every token of every run of >= 2 exactly once and no token of a unit run, the row map is the flatten, the largest kv_end is right, for every
    tile width 1 .. 64 (1 and 2 are new with this option), 256 runs, T = 1024: tests/xm_tiles_check.cpp with its own main, compiled alone with
    -fsanitize=address,undefined and run as a child process (nothing sanitized is loaded into Python)"""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "xm_tiles_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                           "-I", CSRC, "-o", exe, os.path.join(ROOT, "tests", "xm_tiles_check.cpp")])      # runtimes inside the program: no library order to get wrong
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert run.returncode == 0 and "xm tiles ok" in run.stdout, run.stdout
