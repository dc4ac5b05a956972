"""The "multi_extend_la_exact" option (docs/design/36-multi-extend-la-exact.md) without a GPU: both options are parsed and documented in every layer, the refusal
is the last rule of the ordered rule list, asked behind the "multi_mla_exact_split" rule, the four kernels are one text in the device header with two callers, the run kernels leave a staged run
ahead of their first barrier, the new field of KrMultiLaArgs stands ahead of the chunked rule's, no C-ABI symbol was added, and the table builder and the plan
pass their stand-alone check under AddressSanitizer and UBSan in a child process."""
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "krasis_amd", "csrc")
OPT, MIN = "multi_extend_la_exact", "multi_extend_la_exact_min"
DOC = "36-multi-extend-la-exact.md"
KERNELS = ("kr_pfm_la_conv_kernel", "kr_pfm_la_conv_state_kernel", "kr_pfm_la_recur_kernel", "kr_pfm_gated_norm_kernel")


def _src(name):
    return open(os.path.join(CSRC, name)).read()


def _code(text):
    return re.sub(r"//.*", "", text)


def _body(src, head):
    body = src[src.index(head):]
    return body[:body.index("\n}\n")]


def _lib():
    from krasis_amd import _lib
    if not os.path.exists(_lib.lib_path()):
        subprocess.check_call(["make", "-C", CSRC])
    return _lib


def test_the_options_are_parsed_and_documented():
    from tests.util import option_field
    dec = _src("kr_decode.cpp")
    for o in (OPT, MIN):
        assert '!strcmp(name, "%s")' % o in dec and option_field(o) == o[len("multi_"):]
    parse = dec[dec.index('"%s"))' % MIN):][:400]
    assert "if (value < 2 || value > 1024) return kr_fail(KR_ERR_VALUE" in parse and MIN in parse[20:]      # 2 .. 1024, the message names the option
    assert re.search(r"int extend_la_exact = 0;", _src("kr_multi_opts.h")) and re.search(r"int extend_la_exact_min = 8;", _src("kr_multi_opts.h"))                                 # off by default
    header = open(os.path.join(ROOT, "include", "krasis_hip.h")).read()
    assert '"%s"' % OPT in header and '"%s"' % MIN in header and DOC in header
    from krasis_amd.decode_store import CpuDecodeStore
    assert MIN in CpuDecodeStore.set_option.__doc__
    for fn in (CpuDecodeStore.set_option, CpuDecodeStore.extend_multi, CpuDecodeStore.prefill_slot):
        assert OPT in fn.__doc__, fn.__name__
    doc = open(os.path.join(ROOT, "docs", "design", DOC)).read()
    for head in ("## Contract", "## Refusals", "## Kernels", "## Bounds", "## Resources", "## Measured", "## Out of scope"):
        assert head in doc, head
    for word in (OPT, MIN, "kernel-resource-usage", "vmcnt(7)", "kr_m_run_row", "phantom") + KERNELS:
        assert word in doc, word
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert OPT in readme and MIN in readme
    assert OPT in open(os.path.join(ROOT, "DESIGN.md")).read() and "kr_multi_la_exact.hip" in open(os.path.join(ROOT, "DESIGN.md")).read()
    for older in ("17-multi-extend.md", "28-multi-extend-exact-mfma.md"):
        assert DOC in open(os.path.join(ROOT, "docs", "design", older)).read(), older
    assert os.path.exists(os.path.join(ROOT, "profiles", "multi_extend_la_exact.txt"))
    probe = open(os.path.join(ROOT, "tools", "probes", "multi_extend_throughput.py")).read()
    assert '"--la-exact" in sys.argv' in probe and '"%s"' % OPT in probe


def test_the_refusal_is_a_function_of_its_own_behind_its_siblings():
    from tests.util import FLAGS, recorded_refusal, rule_place_seen, rule_row
    pre = _src("kr_decode_prefill.cpp")
    span = pre[pre.index("int kr_exact_refuse("):pre.index("int kr_spec_refuse(")]
    assert OPT not in span and "multi_extend" not in span                     # kr_exact_refuse holds the base clauses only
    row = rule_row(OPT)
    assert row.startswith('{"multi_extend_la_exact", &KrMultiOpts::extend_la_exact, ATTN_LA, true, "multi_extend_la_chunk", &KrMultiOpts::extend_la_chunk, "the long runs of the linear-attention layers", 0, false, "",')
    assert re.search(r"KR_ERR_VALUE[^;]*not covered", row) and row.count("kr_fail(") == 1 and row.count(OPT) == 2 and row.rstrip().endswith("nullptr, nullptr},")      # the row's name, which the walk puts into both KR_ERR_STATE messages, and the geometry message; nothing to prepare
    assert "kr_multi_lx_ok(L.dk, L.dv, L.nk, L.nv, s->weights[L.qkvz_wid]->rows)" in row
    assert pre.count("bool paged_refused(") == 1 and pre.count("for (const KrOptRule& r : kr_opt_rules)") == 1 and "(r.stand_back && back)) continue;" in pre      # one predicate, one walker: stands back where the entry point's paged refusal applies
    body = _body(_src("kr_decode_multi.cpp"), "int multi_refuse(kr_decode_store* s) {")
    order = [body.index(c) for c in ("kr_spec_pending_fail(s)", "kr_exact_refuse(s, true)", "return kr_option_rules(s, false);")]
    assert order == sorted(order)
    # the last rule of the list: asked only when every sibling ahead of it passed, "multi_mla_exact_split" among them; both options: the message names both
    assert FLAGS[-1] == OPT and rule_place_seen(OPT) >= 8
    assert recorded_refusal("gqa/flat", "multi_mla_exact_split", OPT) == recorded_refusal("gqa/flat", "multi_mla_exact_split") != recorded_refusal("gqa/flat", OPT)
    assert recorded_refusal("la/flat", OPT, "multi_extend_la_chunk") == 'RuntimeError: the "multi_extend_la_exact" and "multi_extend_la_chunk" options both claim the long runs of the linear-attention layers: set one of them to 0'
    assert recorded_refusal("gqa/flat", OPT) == 'RuntimeError: the "multi_extend_la_exact" option covers linear-attention layers only: this store has none (set the option to 0)'
    assert recorded_refusal("la/flat", OPT) == "ok" and recorded_refusal("hybrid/paged", OPT) == "ok" and recorded_refusal("hybrid-dk64/flat", OPT) == "ok"
    # the geometry rule is kr_launch_pfm_la's
    lx = _src("kr_multi_la_exact.hip")
    assert "return (dk == 64 || dk == 128) && dv >= dk && dv <= 256 && dv % 8 == 0 && nk >= 1 && nv == nk * (nv / nk) && ld_qkvz % 4 == 0;" in lx


def test_one_text_two_callers():
    """the four kernels are kernel templates in the device header; the prompt pass instantiates them with an identity placement and names no slot and no table,
    the batched pass with the placement of a tile / run of its tables"""
    dev = _src("kr_pfm_la_dev.h")
    code = _code(dev)
    assert code.count("__global__") == 4
    for k in KERNELS:
        assert len(re.findall(r"\b%s\(" % k, code)) == 1, k                   # defined once, launched elsewhere
    assert re.search(r"template <class Where>\s*__global__ void __launch_bounds__\(256\) kr_pfm_la_conv_kernel\(typename Where::ConvArgs A\)", dev)
    assert re.search(r"template <class Where>\s*__global__ void kr_pfm_la_conv_state_kernel\(typename Where::ConvArgs A\)", dev)
    assert re.search(r"template <int DK, class Where>\s*__global__ void __launch_bounds__\(256\) kr_pfm_la_recur_kernel\(typename Where::RecurArgs A\)", dev)
    assert re.search(r"template <class Where>\s*__global__ void __launch_bounds__\(256\) kr_pfm_gated_norm_kernel\(", dev) and "typename Where::NormPlace P" in dev
    assert code.count("W.row(") == 9 and "W.cs(a)" in code               # conv: the window, v, z, the gates, q | k; conv state; the ring's requests and the output; the norm
    assert "W.cs(a)" in code and "W.state(R)" in code
    assert code.count("asm volatile") == 3 and code.count("global_load_lds_dword") == 1      # the DMA helper and the two waits the body always had: nothing new
    for word in ("runs", "kr_m_run_row", "lx_", "t16", "conv_stride", "recur_stride"):      # (`slot` there is a slot of the delta rule's LDS ring)
        assert not re.search(r"\b%s" % word, code), word                      # the shared text knows no placement of its own
    # the delta rule's loop: five requests per token and wave, one wait, one barrier, the output through the row map
    loop = code[code.index("for (int t = 0; t < C; t++) {"):]
    loop = loop[:loop.index("__builtin_amdgcn_raw_buffer_store_b32")]
    assert loop.count("request(") == 1 and loop.count("__syncthreads()") == 1 and loop.count('s_waitcnt vmcnt(7)') == 1
    assert "out[(size_t)W.row(t) * nvdv + (size_t)h * dv + j] = ob;" in loop
    req = code[code.index("auto request = [&]"):code.index("request(0, 0);")]
    assert req.count("pfm_dma4(") == 5 and "W.row(tt < C ? tt : C - 1)" in req                # the phantom token re-reads the last row
    single = _src("kr_prefill_ops.hip")
    scode = _code(single)
    assert '#include "kr_pfm_la_dev.h"' in single and "global_load_lds_dword" not in single      # the bodies moved whole
    assert "struct KrPfmLaSeq {" in single and "int row(int t) const { return t; }" in single
    assert "float* cs(const KrPfmLaArgs& a) const { return a.conv_state; }" in single and "float* state(const KrPfmLaRecurArgs& r) const { return r.state; }" in single
    for k, n in (("kr_pfm_la_conv_kernel<KrPfmLaSeq>", 1), ("kr_pfm_la_conv_state_kernel<KrPfmLaSeq>", 1), ("kr_pfm_gated_norm_kernel<KrPfmLaSeq>", 2),
                 ("kr_pfm_la_recur_kernel<128, KrPfmLaSeq>", 2), ("kr_pfm_la_recur_kernel<64, KrPfmLaSeq>", 2)):
        assert scode.count(k) == n, k
    for grid in ("dim3(a.nk, (C + PFC_WT - 1) / PFC_WT), dim3(256), (size_t)(2 * PFC_WT * a.dk + 2 * PFC_WT) * 4", "dim3((conv_dim + 255) / 256), dim3(256), 0",
                 "dim3(a.nv), dim3(a.dv), 0", "dim3(a.nv, (C + PFG_TT - 1) / PFG_TT), dim3(256), 0"):
        assert grid in single, grid                                           # launched as before
    la = scode[scode.index("struct KrPfmLaSeq {"):scode.index("__global__ void __launch_bounds__(256) kr_pfm_gqa_prep_kernel")]
    for word in ("slot", "page", "table", "runs", "kr_multi"):
        assert not re.search(r"\b%s" % word, la), word                        # the single-sequence side names no slot and no table
    multi = _src("kr_multi_la_exact.hip")
    mcode = _code(multi)
    assert '#include "kr_pfm_la_dev.h"' in multi and "struct KrPfmLaSlot {" in multi and "__global__" not in mcode      # no kernel text of its own
    assert "int row(int t) const { return kr_m_run_row(run, off, C, t); }" in multi       # the flatten of 17-multi-extend.md, conv window included
    assert "return a.conv_state + (size_t)slot * stride;" in multi and "return r.state + (size_t)slot * stride;" in multi
    assert "asm" not in mcode and "hipGraph" not in multi and "extern __shared__" not in mcode and "kr_lds_optin" not in multi
    launch = multi[multi.index("int kr_launch_multi_la_exact("):]
    order = [launch.index(k) for k in ("kr_pfm_la_conv_kernel<KrPfmLaSlot>", "kr_pfm_la_conv_state_kernel<KrPfmLaSlot>", "kr_pfm_la_recur_kernel<128, KrPfmLaSlot>",
                                       "kr_pfm_gated_norm_kernel<KrPfmLaSlot>")]
    assert order == sorted(order)                                             # the carried conv inputs advance behind the conv launch
    for grid in ("dim3(m.nk, x.n16), dim3(256)", "dim3((conv_dim + 255) / 256, x.n_runs), dim3(256)", "dim3(m.nv, x.n_runs), dim3(m.dv)", "dim3(m.nv, x.n8), dim3(256)"):
        assert grid in launch, grid
    assert launch.index("if (!kr_multi_lx_args_ok(m, x)) return 1;") < launch.index("hipLaunchKernelGGL")      # every check ahead of the first launch
    mk = _src("Makefile")
    assert "kr_multi_la_exact.hip" in mk and "kr_pfm_la_dev.h" in mk


def test_the_run_kernels_leave_staged_runs_and_option_off_launches_what_it_launched():
    hdr = _src("kr_multi.h")
    body = re.search(r"struct KrMultiLaArgs \{(.*?)\n\};", hdr, re.S).group(1)
    assert body.index("float *rec_x, *rec_k, *rec_v, *rec_ge, *rec_be;") < body.index("int lx_min;") < body.index("const int* lc_runs;")
    assert body.rstrip().endswith("const int* lc_runs; const int* lc_tiles; int lc_nruns, lc_ntiles, lc_short; float* lc_scratch; float* lc_o;")
    assert "return a.lx_min && cnt >= a.lx_min;" in hdr                       # 0: no run is skipped
    multi = _src("kr_multi.hip")
    conv = multi[multi.index("kr_multi_la_conv_kernel(const KrMultiLaArgs a"):multi.index("#define KR_M_RUN_MAX")]
    assert "if constexpr (!VERIFY) if (kr_m_run_staged(a, cnt)) return;" in conv and "__syncthreads" not in _code(conv)
    recur = multi[multi.index("kr_multi_la_recur_kernel(const KrMultiLaArgs a"):]
    assert recur.index("if (kr_m_run_chunked(a, cnt)) return;") < recur.index("if constexpr (!VERIFY) if (kr_m_run_staged(a, cnt)) return;") < recur.index("__syncthreads()")
    launch = multi[multi.index("int kr_launch_multi_la("):multi.index("// ---- softmax of one score row")]
    verify = launch[:launch.index("return 0;")]
    assert "lx_" not in verify and "x->" not in verify                        # the verify form is untouched
    assert launch.index("kr_multi_lx_args_ok(a, *x)") < launch.index("kr_multi_la_conv_kernel<false>")      # every check ahead of the first launch
    assert "if (x && x->n_short == 0) return kr_launch_multi_la_exact(a, *x, runs, st);" in launch           # not launched when every run is staged
    assert launch.index("x->n_short == 0") < launch.index("kr_multi_la_conv_kernel<false>") < launch.index("if (x) return kr_launch_multi_la_exact(a, *x, runs, st);")
    pre = _src("kr_decode_prefill.cpp")
    assert "if (pl.lx_nruns) m.lx_min = s->mopt.extend_la_exact_min;" in pre and "cx.mp->plan.lx_nruns ? &x : nullptr" in pre      # option off: 0 and null
    assert "o.opt = s->mopt;" in pre[pre.index("int kr_multi_pass("):]
    plan = _src("kr_multi_plan.h")
    assert "o.opt.extend_la_exact && !r.verify && r.counts && nv_max" in plan and "o.opt.extend_la_exact_min, xr, x16, x8)" in plan and _code(plan).count("kr_lx_build(") == 1
    opts = re.search(r"struct KrMultiOpts \{(.*?)\n\};", _src("kr_multi_opts.h"), re.S).group(1)
    assert [l.strip().split(";")[0] for l in opts.rstrip().splitlines()[-2:]] == ["int extend_la_exact = 0", "int extend_la_exact_min = 8"]      # behind the fields existing callers may name in order
    assert "KrMpSpan lx_runs, lx_t16, lx_t8;" in plan
    tiles = _code(_src("kr_lc_tiles.h"))
    assert "inline KrLxStats kr_lx_build(" in tiles and "hip" not in tiles.lower() and "__device__" not in tiles


def test_library_exports_no_new_symbol_and_holds_the_new_kernels():
    lib = _lib()
    out = subprocess.run(["nm", "-D", "--defined-only", lib.lib_path()], stdout=subprocess.PIPE, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if re.search(r" T kr_\w+$", line)}
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "krasis_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(kr_\w+)\s*\(", header))
    assert not exported - declared, sorted(exported - declared)
    assert not [n for n in exported if "la_exact" in n or "multi_lx" in n or "kr_lx" in n or "pfm_la" in n]
    names = subprocess.run(["nm", "-C", lib.lib_path()], stdout=subprocess.PIPE, text=True, check=True).stdout
    assert "kr_launch_multi_la_exact" in names                                # the feature is in the library
    for k in ("kr_pfm_la_conv_kernel<%s>", "kr_pfm_la_conv_state_kernel<%s>", "kr_pfm_la_recur_kernel<128, %s>", "kr_pfm_la_recur_kernel<64, %s>", "kr_pfm_gated_norm_kernel<%s>"):
        for where in ("KrPfmLaSeq", "KrPfmLaSlot"):
            assert k % where in names, (k, where)


def test_table_program_under_sanitizers(tmp_path):
    """a plain step and a verify pass have no table; runs at min - 1, min, 16, 17 and 1024; several staged runs; tile counts and order; the count of runs left
    to the run kernels: tests/la_exact_tiles_check.cpp with its own main, compiled alone with -fsanitize=address,undefined and run as a child process (nothing
    sanitized is loaded into Python)"""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "la_exact_tiles_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                           "-I", CSRC, "-o", exe, os.path.join(ROOT, "tests", "la_exact_tiles_check.cpp")])      # runtimes inside the program: no library order to get wrong
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert run.returncode == 0 and "la exact tiles ok" in run.stdout, run.stdout
