"""The "multi_extend_la_chunk" option (docs/design/26-multi-extend-la-chunk.md) without a GPU: the option is known in every layer, the single-sequence prompt pass
and the batched runs share the two kernel templates of the chunked delta rule, the refusal clause is the last one and names the option, the new fields of
KrMultiLaArgs stand at its end, no C-ABI symbol was added, and the table builder -- a host-only header -- passes its stand-alone check under AddressSanitizer and
UBSan in a child process."""
import os
import re
import shutil
import subprocess

from tests.test_multi_pass_plan import case_passed

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "krasis_amd", "csrc")
OPT = "multi_extend_la_chunk"
DOC = "26-multi-extend-la-chunk.md"


def _src(name):
    return open(os.path.join(CSRC, name)).read()


def _code(text):
    return re.sub(r"//.*", "", text)


def test_the_option_is_known_everywhere():
    assert '!strcmp(name, "%s")' % OPT in _src("kr_decode.cpp")
    from tests.util import option_field
    assert option_field(OPT) == "extend_la_chunk"
    header = open(os.path.join(ROOT, "include", "krasis_hip.h")).read()
    assert '"%s"' % OPT in header and DOC in header
    from krasis_amd.decode_store import CpuDecodeStore
    for fn in (CpuDecodeStore.set_option, CpuDecodeStore.extend_multi, CpuDecodeStore.prefill_slot):
        assert OPT in fn.__doc__, fn.__name__
    for fn in (CpuDecodeStore.extend_multi, CpuDecodeStore.set_option):
        assert ">= 64" in fn.__doc__ and "sub-chunk" in fn.__doc__, fn.__name__      # the cut-dependence note
    doc = open(os.path.join(ROOT, "docs", "design", DOC)).read()
    for head in ("## Contract", "## Kernels", "## Resources", "## Measured", "## Out of scope"):
        assert head in doc, head
    assert OPT in open(os.path.join(ROOT, "docs", "design", "02-numerics.md")).read()
    assert OPT in open(os.path.join(ROOT, "README.md")).read()
    for older in ("17-multi-extend.md", "25-multi-extend-flash.md"):
        assert DOC in open(os.path.join(ROOT, "docs", "design", older)).read(), older


def test_one_body_two_callers():
    """both kernels are kernel templates in the device header; the prompt pass instantiates them with an identity placement and names no slot and no table, the
    batched pass with the placement of a tile of its table"""
    dev = _src("kr_lac_dev.h")
    for k, lb in (("kr_lac_prep_kernel", "LC_PTH"), ("kr_lac_scan_kernel", "256")):
        m = re.search(r"template <class Where>\s*__global__ void __launch_bounds__\(%s\) %s\(typename Where::Args A\)" % (lb, k), dev)
        assert m, k
    assert dev.count("__global__") == 2 and dev.count("extern __shared__") == 2
    assert "W.row(" in dev and "W.conv(a)" in dev and "W.state(a)" in dev and "W.tile0()" in dev and "W.tile()" in dev
    assert "asm" not in _code(dev)
    for word in ("slot", "lc_tiles", "lc_runs", "kr_m_run_row"):
        assert not re.search(r"\b%s" % word, _code(dev)), word                # the shared text knows no placement of its own
    single = _src("kr_la_chunk.hip")
    code = _code(single)
    assert '#include "kr_lac_dev.h"' in single and "__global__" not in single and "extern __shared__" not in single      # the bodies moved whole
    assert "struct KrLacChunk" in single and "int row(int t) const { return t; }" in single and "int tile0() const { return 0; }" in single
    assert code.count("kr_lac_prep_kernel<KrLacChunk>") == 2 and code.count("kr_lac_scan_kernel<KrLacChunk>") == 2      # the LDS window and the launch
    assert "dim3(a.n_sub, p.nv), dim3(LC_PTH), LC_PREP_LDS" in single and "dim3(p.nv * 4), dim3(256), LC_SCAN_LDS" in single      # launched as before
    for word in ("slot", "page", "table", "lc_tiles", "runs", "kr_multi"):
        assert not re.search(r"\b%s" % word, code), word                      # the single-sequence side names no slot and no table
    multi = _src("kr_multi_la_chunk.hip")
    assert '#include "kr_lac_dev.h"' in multi and "struct KrLacSlot {" in multi
    assert "kr_m_run_row(run, off, C, t)" in multi                            # the flatten of 17-multi-extend.md, conv window included
    assert "A.conv_state + (size_t)slot * A.conv_stride" in multi and "A.recur + (size_t)slot * A.recur_stride" in multi
    assert _code(multi).count("kr_lac_prep_kernel<KrLacSlot>") == 2 and _code(multi).count("kr_lac_scan_kernel<KrLacSlot>") == 2
    assert "dim3(m.lc_ntiles, m.nv), dim3(LC_PTH), LC_PREP_LDS" in multi and "dim3(m.nv * 4, m.lc_nruns), dim3(256), LC_SCAN_LDS" in multi
    launch = multi[multi.index("int kr_launch_multi_la_chunk("):]
    order = [launch.index(k) for k in ("kr_lac_prep_kernel<KrLacSlot>", "kr_multi_lc_conv_state_kernel,", "kr_lac_scan_kernel<KrLacSlot>", "kr_multi_lc_gated_norm_kernel,")]
    assert order == sorted(order)                                             # the carried conv inputs advance behind the prep launch
    assert "kr_lds_optin" not in launch                                       # the windows are not raised inside the pass
    assert "asm" not in _code(multi) and "hipGraph" not in multi
    mk = _src("Makefile")
    assert "kr_multi_la_chunk.hip" in mk and "kr_lac_dev.h" in mk and "kr_lc_tiles.h" in mk


def test_refusal_clause_is_last_and_names_the_option():
    from tests.util import FLAGS, recorded_refusal, rule_row
    pre = _src("kr_decode_prefill.cpp")
    row = rule_row(OPT)
    # stands back where the entry point's paged refusal applies; no rival; "has none" ahead of the MLA step; geometry last
    assert row.startswith('{"multi_extend_la_chunk", &KrMultiOpts::extend_la_chunk, ATTN_LA, true, nullptr, nullptr, nullptr, 2, false, " for the exact pass",')
    assert FLAGS.index(OPT) == 5 and FLAGS[:5] == ("multi_attn_fast", "multi_attn_fast_paged", "multi_mla_fast", "multi_extend_mla_flash", "multi_extend_flash")      # the last of the tolerance forms; the exact forms stand behind it
    assert row.count(OPT + ":") == 2                                          # geometry, LDS window; "has none" and "is MLA" take the row's name
    assert '"multi_extend_flash"' not in row and "multi_extend_flash:" not in row
    walk = pre[pre.index("int kr_option_rules("):]
    assert re.search(r"KR_ERR_STATE[^;]*this store has none", walk) and re.search(r"KR_ERR_STATE[^;]*layer %zu is MLA", walk)
    assert walk.index("if (r.mla_at == 1)") < walk.index("if (!has_attn(s, r.kind))") < walk.index("if (r.mla_at == 2)")
    assert re.search(r"KR_ERR_VALUE[^;]*not covered", row) and re.search(r"KR_ERR_HIP[^;]*LDS window", row)
    assert "kr_multi_lc_prepare()" in row and row.rstrip().endswith("&kr_multi_state::lc_ready},")      # windows once per slot set, outside the pass
    assert "kr_multi_lc_ok(L.dk, L.dv, L.nk, L.nv," in row
    # as a caller sees it: behind the attention-mode bit, "multi_mla_fast" and "multi_extend_flash"; "has none" on an MLA-only store (not "is MLA"); ahead of
    # every exact form
    none = 'RuntimeError: the "multi_extend_la_chunk" option covers linear-attention layers only: this store has none (set the option to 0 for the exact pass)'
    assert recorded_refusal("mla/flat", OPT) == none and recorded_refusal("gqa/flat", OPT) == none and recorded_refusal("la/flat", OPT) == "ok"
    assert "the attention mode has tolerance bits set" in recorded_refusal("gqa/flat", OPT, mode=True)
    assert 'the "multi_mla_fast" option' in recorded_refusal("gqa/flat", "multi_mla_fast", OPT)
    assert 'the "multi_extend_flash" option covers GQA layers only: layer 0 is MLA' in recorded_refusal("mla/flat", "multi_extend_flash", OPT)
    for later in FLAGS[6:]:
        assert recorded_refusal("gqa/flat" if "mla" in later or "la_exact" in later else "mla/flat", OPT, later) == none, later
    assert recorded_refusal("hybrid-dk64/flat", OPT).startswith("ValueError: multi_extend_la_chunk: linear-attention geometry nk 2 nv 4 dk 64 dv 64 not covered")
    assert recorded_refusal("gqa/paged", "multi_attn_fast", OPT).startswith('RuntimeError: "multi_attn_fast" does not read paged slots')
    assert "return dk == LC_D && dv == LC_D" in _src("kr_multi_la_chunk.hip")
    # the pass: never in a verify pass, the table with the other tables of the pass, the scratch ahead of the layer loop
    assert "o.opt = s->mopt;" in pre and "o.opt.extend_la_chunk && !r.verify && r.counts" in _src("kr_multi_plan.h")
    assert case_passed("F") and case_passed("G") and case_passed("K")      # a plain step and a verify pass have no table (docs/design/32-multi-pass-plan.md)
    p = pre[pre.index("int kr_multi_pass("):]
    assert p.index("kr_multi_plan(o, ") < p.index("M.lc_scratch.ensure(") < p.index("run_layer(s, cx, l)")


def test_new_fields_stand_at_the_end_and_the_run_kernels_leave_chunked_runs():
    hdr = _src("kr_multi.h")
    body = re.search(r"struct KrMultiLaArgs \{(.*?)\n\};", hdr, re.S).group(1)
    assert "float *rec_x, *rec_k, *rec_v, *rec_ge, *rec_be;" in body
    assert body.rstrip().endswith("const int* lc_runs; const int* lc_tiles; int lc_nruns, lc_ntiles, lc_short; float* lc_scratch; float* lc_o;")
    assert "return a.lc_runs && cnt >= KR_M_LC_MIN;" in hdr and "#define KR_M_LC_MIN 64" in hdr      # null pointer: no run is skipped
    multi = _src("kr_multi.hip")
    conv = multi[multi.index("kr_multi_la_conv_kernel(const KrMultiLaArgs a"):multi.index("#define KR_M_RUN_MAX")]
    assert "if (kr_m_run_chunked(a, cnt)) return;" in conv and "__syncthreads" not in _code(conv)
    recur = multi[multi.index("kr_multi_la_recur_kernel(const KrMultiLaArgs a"):]
    assert recur.index("if (kr_m_run_chunked(a, cnt)) return;") < recur.index("__syncthreads()")      # ahead of the first barrier
    launch = multi[multi.index("int kr_launch_multi_la("):multi.index("// ---- softmax of one score row")]
    assert "if (!a.lc_runs || a.lc_short > 0) {" in launch                   # not launched when every run is chunked
    assert launch.index("kr_multi_lc_ok(") < launch.index("kr_multi_la_conv_kernel<false>")      # every check ahead of the first launch
    assert "if (a.lc_runs) return kr_launch_multi_la_chunk(a, runs, st);" in launch
    verify = launch[:launch.index("return 0;")]
    assert "lc_" not in verify                                               # the verify form is untouched


def test_the_table_builder_is_host_only():
    code = _code(_src("kr_lc_tiles.h"))
    assert "hip" not in code.lower() and "__device__" not in code
    assert '#include "kr_lc_tiles.h"' in _src("kr_multi_plan.h") and '#include "kr_multi_plan.h"' in _src("kr_decode_prefill.cpp")


def test_library_exports_no_new_symbol():
    from krasis_amd import _lib
    if not os.path.exists(_lib.lib_path()):
        subprocess.check_call(["make", "-C", CSRC])
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.lib_path()], stdout=subprocess.PIPE, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if re.search(r" T kr_\w+$", line)}
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "krasis_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(kr_\w+)\s*\(", header))
    assert not exported - declared, sorted(exported - declared)
    assert not [n for n in exported if "la_chunk" in n or "multi_lc" in n or "lc_tiles" in n or "kr_lac" in n]
    out = subprocess.run(["nm", "-C", _lib.lib_path()], stdout=subprocess.PIPE, text=True, check=True).stdout
    assert "kr_launch_multi_la_chunk" in out                                  # the feature is in the library


def test_table_program_under_sanitizers(tmp_path):
    """every token of every run of >= 64 in exactly one sub-chunk and no token of a shorter run, partial last sub-chunks, the scratch prefixes and size, 256 runs,
    one run of 1024 tokens: tests/lc_tiles_check.cpp with its own main, compiled alone with -fsanitize=address,undefined and run as a child process (nothing
    sanitized is loaded into Python)"""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "lc_tiles_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                           "-I", CSRC, "-o", exe, os.path.join(ROOT, "tests", "lc_tiles_check.cpp")])      # runtimes inside the program: no library order to get wrong
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert run.returncode == 0 and "lc tiles ok" in run.stdout, run.stdout
