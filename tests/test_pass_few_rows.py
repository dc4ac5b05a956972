"""The "pass_few_rows" option (docs/design/34-pass-few-rows.md) without a GPU: the plan header is host only and passes its stand-alone check under
AddressSanitizer and UBSan in a child process; the pass decides once, through that header; pf_gemm / pf_gemm_multi are the only doors to the few-row launcher;
the kernel file calls the decode matvec's device functions instead of restating them; the new entry point is declared, bound and exported."""
import functools
import os
import re
import shutil
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "krasis_amd", "csrc")
CHECK = os.path.join(ROOT, "tests", "rows_plan_check.cpp")


def _src(name):
    return open(os.path.join(CSRC, name)).read()


def _code(name):
    return re.sub(r"//.*", "", _src(name))


@functools.lru_cache(maxsize=None)
def plan_check():
    """(source text of tests/rows_plan_check.cpp, its output): compiled alone with -fsanitize=address,undefined and run as a child process (nothing sanitized is
    loaded into Python); asserts that it passed"""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "rows_plan_check")
        subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                               "-I", CSRC, "-o", exe, CHECK])      # runtimes inside the program: no library order to get wrong
        run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert run.returncode == 0 and "rows plan ok" in run.stdout, run.stdout
    return open(CHECK).read(), run.stdout


def test_the_plan_program_under_sanitizers():
    src, out = plan_check()
    for letter in "ABCDEFG":      # A: T on both sides of the maximum, B: the KR_GEMM_FAST bit, E: a K whose 16 images do not fit, G: every row in exactly one group
        assert "// case %s: " % letter in src and "case %s ok" % letter in out, letter


def test_the_plan_header_is_host_only():
    src, code = _src("kr_rows_plan.h"), _code("kr_rows_plan.h")
    assert "hip" not in code.lower() and "__device__" not in code and "__global__" not in code
    assert set(re.findall(r"#include [<\"]([^>\"]+)[>\"]", src)) == {"stddef.h"}
    assert "kr_rows_plan.h" in _src("Makefile") and "kr_rows_matvec.hip" in _src("Makefile")
    assert '#include "kr_rows_plan.h"' not in _src("kr_multi_plan.h")      # that header's include set is pinned by its own test
    assert "#define KR_ROWS_MAX 16" in src


def test_the_pass_decides_once_and_through_the_header():
    pre = _code("kr_decode_prefill.cpp")
    assert '#include "kr_rows_plan.h"' in _src("kr_decode_prefill.cpp")
    assert pre.count("kr_rows_use(") == 1                                  # one predicate ...
    assert pre.count("pass_few_rows(s, ") == 2                             # ... asked once by the prompt / verify pass and once by the batched pass
    impl = pre[pre.index("static int prefill_impl("):pre.index('extern "C" int kr_decode_prefill(')]
    assert impl.count("pass_few_rows(s, n_tokens)") == 1 and impl.index("pass_few_rows(s, n_tokens)") < impl.index("for (int c = 0; c < n_chunks; c++)")      # per pass, never per chunk
    multi = pre[pre.index("int kr_multi_pass("):]
    assert multi.count("pass_few_rows(s, n)") == 1
    layer = pre[pre.index("static int run_layer("):pre.index("static void run_final(")]
    assert "opt_pass_few_rows" not in layer and "kr_rows_" not in layer    # a layer reads the decision, it takes none
    assert "(B.few ? KR_PF_SET_ROWS : 0)" in layer


def test_pf_gemm_and_pf_gemm_multi_are_the_only_doors_to_the_launcher():
    pre = _code("kr_decode_prefill.cpp")
    assert pre.count("kr_launch_rows_matvec(") == 1
    few = pre[pre.index("static int pf_few("):pre.index("static int pf_gemm(")]
    assert "kr_launch_rows_matvec(" in few
    assert pre.count("pf_few(") == 3                                       # its definition, pf_gemm, pf_gemm_multi
    gemm = pre[pre.index("static int pf_gemm("):pre.index("static int pf_gemm_multi(")]
    multi = pre[pre.index("static int pf_gemm_multi("):pre.index("static void pf_rows(")]
    assert gemm.count("pf_few(") == 1 and multi.count("pf_few(") == 1
    # the producers launch nothing for a few-row pass: the kernel quantises (and activates) in its prologue
    rows = pre[pre.index("static void pf_rows("):pre.index("static void pf_act(")]
    act = pre[pre.index("static void pf_act("):pre.index("static bool pass_few_rows(")]
    assert rows.index("if (B.few") < rows.index("kr_launch_pfm_quant_f32(") and act.index("if (B.few") < act.index("kr_launch_pf_act(")
    # the only other caller of the launcher is the stand-alone operator
    callers = [n for n in os.listdir(CSRC) if n.endswith((".cpp", ".hip")) and "kr_launch_rows_matvec(" in _code(n)]
    assert sorted(callers) == ["kr_decode_prefill.cpp", "kr_decode_standalone.cpp", "kr_rows_matvec.hip"]


def test_the_kernel_calls_the_decode_matvecs_device_functions():
    dev, hip = _code("kr_rows_dev.h"), _code("kr_rows_matvec.hip")
    for fn in ("kr_group_i4(", "kr_group_i8(", "kr_red8_add_i32(", "kr_chain("):
        assert fn in dev, fn
    for fn in ("kr_prologue_quant<", "kr_prologue_hidden<KR_ACT_SILU_MUL", "kr_rows_tile<", "kr_lds_optin(", "kr_rows_plan("):
        assert fn in hip, fn
    for text in (dev, hip):                                                # no dot product, fma chain or quantiser of its own
        for banned in ("sdot4", "udot4", "__builtin_fmaf", "fmaf(", "roundf", "kr_quant8", "kr_group_scale", "32767"):
            assert banned not in text, banned
    # the functions it calls have one definition each, in the headers the decode kernels include
    tile = _code("kr_matvec_tile_dev.h")
    assert tile.count("float kr_chain(") == 1 and tile.count("void kr_prologue_quant(") == 1 and tile.count("void kr_prologue_hidden(") == 1
    moe = _code("kr_moe_decode.hip")
    assert '#include "kr_matvec_tile_dev.h"' in _src("kr_moe_decode.hip")
    for fn in ("float kr_chain(", "void kr_prologue_quant(", "void kr_prologue_hidden(", "float kr_matvec_tile("):
        assert fn not in moe, fn


def test_the_routed_experts_take_the_decode_launches_under_the_rows_bit():
    eng, hdr = _code("kr_engine.cpp"), _src("kr_engine_internal.h")
    assert "#define KR_PF_SET_ROWS 0x800" in hdr and "#define KR_PF_SET_FAST 0x100" in hdr
    body = eng[eng.index("int kr_moe_prefill_set("):eng.index("int kr_moe_prefill_rows(")]
    assert "few_rows = set & KR_PF_SET_ROWS" in body
    rows = body.index("if (few_rows && M <= 16 && !use_shared)")
    assert body.index("return moe_prefill_gguf_exact(") < rows and body.index("return moe_prefill_fast(") < rows      # GGUF layers and the tolerance GEMMs keep their paths
    assert rows < body.index("kr_launch_pf_sort(idc, mc, topk, E, so, st);")
    assert "kr_launch_moe_decode(a, st);" in body[rows:body.index("kr_launch_pf_sort(idc, mc, topk, E, so, st);")]
    assert "KR_PF_SET_ROWS" not in _code("kr_ep.cpp")                      # expert-parallel engines keep their routed path


def test_the_option_and_the_entry_point_are_declared_bound_and_documented():
    dec = _src("kr_decode.cpp")
    for name in ("pass_few_rows", "pass_few_rows_max", "pass_few_rows_group"):
        assert '!strcmp(name, "%s")' % name in dec, name
    assert "value < 1 || value > 16" in dec
    hdr = open(os.path.join(ROOT, "include", "krasis_hip.h")).read()
    assert "int kr_decode_matmul_rows(kr_decode_store* s, int weight_id, const float* input, int n_rows, float* output);" in hdr
    assert '"pass_few_rows"' in hdr and '"pass_few_rows_max"' in hdr and "34-pass-few-rows.md" in hdr
    import krasis_amd._lib as lib_mod
    from krasis_amd.decode_store import CpuDecodeStore
    assert "kr_decode_matmul_rows" in lib_mod.SYMBOLS and hasattr(CpuDecodeStore, "matmul_rows")
    assert os.path.exists(os.path.join(ROOT, "docs", "design", "34-pass-few-rows.md"))
    for doc in ("12-speculative.md", "13-multi-sequence.md"):
        assert "34-pass-few-rows.md" in open(os.path.join(ROOT, "docs", "design", doc)).read(), doc
    assert "pass_few_rows" in open(os.path.join(ROOT, "README.md")).read()


def test_the_library_exports_the_entry_point():
    from krasis_amd import _lib
    if not os.path.exists(_lib.lib_path()):
        subprocess.check_call(["make", "-C", CSRC])
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.lib_path()], stdout=subprocess.PIPE, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if re.search(r" T kr_\w+$", line)}
    assert "kr_decode_matmul_rows" in exported
    assert not [n for n in exported if "rows_matvec" in n or "kr_rows_" in n]      # the launcher stays internal
