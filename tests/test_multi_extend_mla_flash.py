"""The "multi_extend_mla_flash" option (docs/design/27-multi-extend-mla-flash.md) without a GPU: the option is known in every layer, the MLA flash body is one
device function with a row-map parameter whose default is the identity, the single-sequence kernel names no slot, run or table, the run kernel calls the body in
its flat and its paged form through the flatten of the pass, the refusal clause stands between the "multi_mla_fast" clause and the clauses of the two other run
options, the new fields stand at the end of KrMultiMlaArgs, the three per-row kernels leave a row of a longer run ahead of their first barrier, no C-ABI symbol
was added, and the tile-table builder -- a host-only header -- passes its stand-alone check under AddressSanitizer and UBSan in a child process."""
import os
import re
import shutil
import subprocess

from tests.test_multi_pass_plan import case_passed

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "krasis_amd", "csrc")
OPT = "multi_extend_mla_flash"
DOC = "27-multi-extend-mla-flash.md"


def _src(name):
    return open(os.path.join(CSRC, name)).read()


def _code(text):
    return re.sub(r"//[^\n]*", "", text)


def test_the_option_is_known_everywhere():
    assert '!strcmp(name, "%s")' % OPT in _src("kr_decode.cpp")
    from tests.util import option_field
    assert option_field(OPT) == "extend_mla_flash"
    header = open(os.path.join(ROOT, "include", "krasis_hip.h")).read()
    assert header.count('"%s"' % OPT) >= 2 and DOC in header               # the option's paragraph and kr_decode_extend_multi's comment
    from krasis_amd.decode_store import CpuDecodeStore
    for fn in (CpuDecodeStore.set_option, CpuDecodeStore.extend_multi, CpuDecodeStore.prefill_slot):
        assert OPT in fn.__doc__, fn.__name__
    for fn in (CpuDecodeStore.extend_multi, CpuDecodeStore.set_option):
        assert "alone" in fn.__doc__ and ">= 2" in fn.__doc__, fn.__name__      # the cut-dependence note
    doc = open(os.path.join(ROOT, "docs", "design", DOC)).read()
    for section in ("## Contract", "## Kernels", "## Resources", "## Measured", "## Out of scope"):
        assert section in doc, section
    assert OPT in open(os.path.join(ROOT, "docs", "design", "02-numerics.md")).read()
    assert OPT in open(os.path.join(ROOT, "README.md")).read()


def test_one_body_with_a_row_map_and_two_kinds_of_caller():
    dev = _src("kr_mla_flash_dev.h")
    body = re.search(r"template <([^>]*)>\s*__device__ __forceinline__ void kr_mla_flash_body\(([^)]*)\)", dev)
    assert body and "bool SPLIT" in body.group(1) and "bool PAGED = false" in body.group(1)
    assert body.group(1).rstrip().endswith("class RowMap = KrMfRowsIdentity")      # one more trailing template parameter, identity by default
    assert body.group(2).rstrip().endswith("RowMap rmap = {}")               # one more trailing function parameter
    ident = dev[dev.index("struct KrMfRowsIdentity"):dev.index("};", dev.index("struct KrMfRowsIdentity"))]
    assert "operator()(int row) const { return row; }" in ident
    code = _code(dev)
    assert code.count("kr_mla_flash_body(") == 1                             # one device function
    assert code.count("rmap(") == 2 and "rmap(gr)" in code and "rmap(myrow)" in code      # the query load and the attn_lat store, nothing else
    for local in ("const int p_q = pos0 + (row_ok ? myrow / nh : 0);", "const int tok_first = row0 / nh, tok_last = min(C - 1, (row0 + MF_ROWS - 1) / nh);",
                  "const int kv_end = pos0 + tok_last + 1"):
        assert local in code, local                                          # positions and masks stay in the caller's own rows
    # the single-sequence file names nothing new
    single = _src("kr_mla_flash.hip")
    call = re.search(r"kr_mla_flash_body<KLR, FP8, SPLIT>\([^;]*;", single)
    assert call and "rmap" not in single and "RowMap" not in single and "KrMf" not in single
    for word in ("slot", "run", "page", "ptab", "mf_tiles", "mf_runs", "table"):
        assert not re.search(r"\b%s" % word, _code(single)), word
    # the run kernel: flat and paged form of the non-SPLIT body, rows through the flatten
    multi = _src("kr_multi_mla_pf_flash.hip")
    kernel = re.search(r"template <([^>]*)>\s*__global__ void __launch_bounds__\(256\) kr_multi_mla_pf_flash_kernel\(const KrMultiMlaArgs a\)", multi)
    assert kernel and kernel.group(1) == "int KLR, bool FP8, bool PAGED"
    assert "kr_mla_flash_body<KLR, FP8, false, true>(" in multi and "kr_mla_flash_body<KLR, FP8, false>(" in multi
    assert "a.page_table + slot * a.page_stride, a.page_shift, rows" in multi
    assert "(const char*)a.ckv_cache + slot * a.ckv_stride, (const char*)a.kpe_cache + slot * a.kpe_stride" in multi
    assert "return kr_m_run_row(run, off, cnt, t) * nh + (g - t * nh);" in multi and "a.positions[kr_m_run_row(run, off, cnt, 0)]" in multi
    kcode = _code(multi[multi.index("kr_multi_mla_pf_flash_kernel(const KrMultiMlaArgs a)"):multi.index("static_assert")])
    assert "return;" not in kcode and "__syncthreads" not in kcode           # every workgroup has a tile: no exit ahead of the body's barriers
    assert "asm" not in _code(multi) and "hipGraph" not in multi
    assert "kr_lds_optin(paged ? multi_mla_pf_fn<true>(klr, fp8) : multi_mla_pf_fn<false>(klr, fp8), lds)" in multi
    for klr in (512, 256):
        for fp8 in ("true", "false"):
            assert "kr_multi_mla_pf_flash_kernel<%d, %s, PAGED>" % (klr, fp8) in multi
    launch = multi[multi.index("int kr_launch_multi_mla_pf_flash("):]
    assert launch.index("if (!kr_multi_mla_pf_args_ok(a)) return 1;") < launch.index("hipLaunchKernelGGL")      # the geometry check ahead of the first launch
    assert "const dim3 grid(a.mf_ntiles);" in launch                         # exactly the tiles of the table
    mk = _src("Makefile")
    assert "kr_multi_mla_pf_flash.hip" in mk and "kr_mf_tiles.h" in mk and "kr_mla_flash_dev.h" in mk


def test_refusal_clause_stands_between_its_neighbours_and_names_the_option():
    from tests.util import FLAGS, recorded_refusal, rule_row
    pre = _src("kr_decode_prefill.cpp")
    row = rule_row(OPT)
    # stands back where the entry point's paged refusal applies; no rival, no MLA step, no geometry rule of its own
    assert row.startswith('{"multi_extend_mla_flash", &KrMultiOpts::extend_mla_flash, ATTN_MLA, true, nullptr, nullptr, nullptr, 0, false, " for the exact pass", nullptr,')
    assert pre.index("bool paged_refused(const kr_decode_store* s) {") < pre.index("int kr_exact_refuse(") < pre.index("int kr_option_rules(")      # the predicate, stated once ahead of its users
    assert FLAGS.index("multi_mla_fast") < FLAGS.index(OPT) < FLAGS.index("multi_extend_flash") < FLAGS.index("multi_extend_la_chunk")      # the order test_multi_pass_plan.py holds the table to
    assert "multi_extend_flash" not in row and "multi_extend_la_chunk" not in row
    assert row.count(OPT + ":") == 1 and re.search(r"KR_ERR_HIP[^;]*LDS window", row)      # LDS window; "has none" takes the row's name
    assert "kr_multi_mla_pf_prepare(L.klr, s->multi->kv_fp8, s->multi->pg.paged())" in row and row.rstrip().endswith("&kr_multi_state::mf_ready},")      # windows once per slot set, outside the pass
    assert "mf_ready" not in pre[pre.index("int kr_multi_pass("):]           # never inside the pass
    assert "if (paged_refused(s))" in _src("kr_decode_multi.cpp") and pre.count("bool paged_refused(") == 1 and pre.count("for (const KrOptRule& r : kr_opt_rules)") == 1      # one predicate, one walker
    # between its neighbours, as a caller sees it on a store that refuses both
    none = 'RuntimeError: the "multi_extend_mla_flash" option covers MLA layers only: this store has none (set the option to 0 for the exact pass)'
    assert recorded_refusal("gqa/flat", OPT) == none and recorded_refusal("mla/flat", OPT) == "ok"
    assert 'the "multi_mla_fast" option covers MLA layers only: this store has none' in recorded_refusal("la/flat", "multi_mla_fast", OPT)
    assert recorded_refusal("la/flat", OPT, "multi_extend_flash") == none and recorded_refusal("gqa/flat", OPT, "multi_extend_la_chunk") == none
    assert "the attention mode has tolerance bits set" in recorded_refusal("gqa/flat", OPT, mode=True)
    assert 'the "multi_attn_fast" option covers GQA layers only' in recorded_refusal("mla/flat", "multi_attn_fast", OPT)
    assert recorded_refusal("gqa/paged", "multi_attn_fast", OPT).startswith('RuntimeError: "multi_attn_fast" does not read paged slots')


def test_new_fields_at_the_end_and_per_row_kernels_leave_longer_runs():
    hdr = _src("kr_multi.h")
    body = re.search(r"struct KrMultiMlaArgs \{(.*?)\n\};", hdr, re.S).group(1)
    assert "const int* page_table; int page_stride, page_shift;" in body and "float *fd_o, *fd_ml; int fd_chunk, fd_chunks;" in body
    assert body.rstrip().endswith("const int* mf_runs; const int* mf_tiles; int mf_nruns, mf_ntiles, mf_units;")
    assert "kr_m_row_in_run(const KrMultiMlaArgs& a, int b) { return a.mf_runs && a.mf_runs[3 * b + 2] >= 2; }" in hdr      # null pointer: no row is skipped
    multi = _src("kr_multi.hip")
    attn = multi[multi.index("kr_multi_mla_attn_kernel(const KrMultiMlaArgs a)"):]
    assert attn.index("if (kr_m_row_in_run(a, row)) return;") < attn.index("__syncthreads()")
    assert attn.index("if (kr_m_row_in_run(a, row)) return;") < attn.index("__builtin_amdgcn_make_buffer_rsrc")      # ahead of the first descriptor too
    flash = _src("kr_multi_mla_flash.hip")
    assert flash.count("if (kr_m_row_in_run(a, b)) return;") == 2
    chunk = flash[flash.index("kr_multi_mla_flash_kernel(const KrMultiMlaArgs a"):]
    assert chunk.index("if (kr_m_row_in_run(a, b)) return;") < chunk.index("kr_mla_flash_body<")
    merge = flash[flash.index("kr_multi_mla_merge_kernel(const KrMultiMlaArgs a"):]
    assert merge.index("if (kr_m_row_in_run(a, b)) return;") < merge.index("kr_fd_merge2_body<KLR>(")
    # the launcher: the run path ahead of the first launch, every check ahead of the prep launch, the per-row kernels over the first rows only
    fn = multi[multi.index("int kr_launch_multi_mla(const KrMultiMlaArgs& a_in"):multi.index("// ---- paged slots: freshly mapped pages read as zero")]
    assert fn.index("if (a.mf_tiles) return multi_mla_runs(a, B, st);") < fn.index("kr_launch_mla_absorb_mfma(")
    runs = multi[multi.index("static int multi_mla_runs(KrMultiMlaArgs& a, int B, hipStream_t st) {"):multi.index("int kr_launch_multi_mla(const KrMultiMlaArgs& a_in")]
    assert runs.index("kr_multi_mla_pf_args_ok(a)") < runs.index("kr_launch_mla_absorb_mfma(") < runs.index("kr_multi_mla_prep_kernel")
    assert "a.mf_nruns);" in runs and "kr_launch_multi_mla_fd(a, a.mf_nruns, st)" in runs and "kr_launch_multi_mla_pf_flash(a, st)" in runs
    assert runs.index("kr_launch_multi_mla_pf_flash(a, st)") < runs.index("kr_launch_mla_wvc_mfma(")
    pre = _src("kr_decode_prefill.cpp")
    assert "o.opt = s->mopt;" in pre and "o.opt.extend_mla_flash ? KR_MP_RUNS_FLASH" in _src("kr_multi_plan.h") and case_passed("F") and case_passed("K")      # never in a verify pass (docs/design/32-multi-pass-plan.md)
    assert case_passed("C") and case_passed("D")                             # the per-row MLA kernels see the unit rows only; a mixed store keeps the score rows


def test_the_tile_builder_is_host_only():
    src = _src("kr_mf_tiles.h")
    code = _code(src)
    assert "hip" not in code.lower() and "__device__" not in code
    assert '#include "kr_mf_tiles.h"' in _src("kr_multi_plan.h") and '#include "kr_multi_plan.h"' in _src("kr_decode_prefill.cpp")


def test_library_exports_exactly_the_declared_symbols():
    """no C-ABI symbol was added: the exported kr_* functions are the ones include/krasis_hip.h declares and krasis_amd._lib binds"""
    from krasis_amd import _lib
    if not os.path.exists(_lib.lib_path()):
        subprocess.check_call(["make", "-C", CSRC])
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.lib_path()], stdout=subprocess.PIPE, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if re.search(r" T kr_\w+$", line)}
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "krasis_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(kr_\w+)\s*\(", header))
    assert not exported - declared, sorted(exported - declared)
    assert set(_lib.SYMBOLS) <= exported
    assert not [n for n in exported if "mla_flash" in n or "mla_pf" in n or "mf_tiles" in n]
    assert any("kr_multi_mla_pf_flash_kernel" in line for line in subprocess.run(["nm", "-C", _lib.lib_path()], stdout=subprocess.PIPE, text=True, check=True).stdout.splitlines())      # the run kernel is in the library


def test_tile_table_program_under_sanitizers(tmp_path):
    """every (token, head) row of every run of >= 2 is in exactly one tile and no row of a unit run is, the row map is the flatten, head counts that do not divide
    64 (3, 5), 64 and 128 heads, 256 runs, T = 1024: tests/mf_tiles_check.cpp with its own main, compiled alone with -fsanitize=address,undefined and run as a
    child process (nothing sanitized is loaded into Python)"""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "mf_tiles_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                           "-I", CSRC, "-o", exe, os.path.join(ROOT, "tests", "mf_tiles_check.cpp")])      # runtimes inside the program: no library order to get wrong
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert run.returncode == 0 and "mf tiles ok" in run.stdout, run.stdout
