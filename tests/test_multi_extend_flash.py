"""The "multi_extend_flash" option (docs/design/25-multi-extend-flash.md) without a GPU: the option is known in every layer, the single-sequence prompt pass
and the batched runs share one kernel template (head_dim 64) and one device function (head_dim 128 / 256), paging is a template parameter, the pinned lines of the batched launcher stand, no C-ABI symbol was
added, and the tile-table builder -- a host-only header -- passes its stand-alone check under AddressSanitizer and UBSan in a child process."""
import os
import re
import shutil
import subprocess

from tests.test_multi_pass_plan import case_passed

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "krasis_amd", "csrc")
OPT = "multi_extend_flash"


def _src(name):
    return open(os.path.join(CSRC, name)).read()


def test_the_option_is_known_everywhere():
    assert '!strcmp(name, "%s")' % OPT in _src("kr_decode.cpp")
    from tests.util import option_field
    assert option_field(OPT) == "extend_flash"
    header = open(os.path.join(ROOT, "include", "krasis_hip.h")).read()
    assert '"%s"' % OPT in header and "25-multi-extend-flash.md" in header
    from krasis_amd.decode_store import CpuDecodeStore
    for fn in (CpuDecodeStore.set_option, CpuDecodeStore.extend_multi, CpuDecodeStore.prefill_slot):
        assert OPT in fn.__doc__, fn.__name__
    for fn in (CpuDecodeStore.extend_multi, CpuDecodeStore.set_option):
        assert "alone" in fn.__doc__ and ">= 2" in fn.__doc__, fn.__name__      # the cut-dependence note
    assert os.path.exists(os.path.join(ROOT, "docs", "design", "25-multi-extend-flash.md"))
    assert OPT in open(os.path.join(ROOT, "docs", "design", "02-numerics.md")).read()
    assert OPT in open(os.path.join(ROOT, "README.md")).read()


def test_refusals_sit_behind_every_earlier_clause_and_name_the_option():
    from tests.util import recorded_refusal, rule_row
    pre = _src("kr_decode_prefill.cpp")
    row = rule_row(OPT)
    # stands back where the entry point's paged refusal applies; no rival; an MLA layer is refused ahead of "has none"; geometry last
    assert row.startswith('{"multi_extend_flash", &KrMultiOpts::extend_flash, ATTN_GQA, true, nullptr, nullptr, nullptr, 1, false, " for the exact pass",')
    assert row.count(OPT + ":") == 2                                           # geometry, LDS window; the two KR_ERR_STATE refusals take the row's name
    assert re.search(r"KR_ERR_VALUE[^;]*not covered", row) and re.search(r"KR_ERR_HIP[^;]*LDS window", row)
    assert "kr_pfm_gqa_flash_ok(L.nh, L.nkv, L.hd)" in row                    # the prompt pass's own geometry rule
    assert "kr_multi_pf_prepare(L.hd, s->multi->kv_fp8, s->multi->pg.paged())" in row and row.rstrip().endswith("&kr_multi_state::pf_ready},")      # windows once per slot set, outside the pass
    walk = pre[pre.index("int kr_option_rules("):]
    assert re.search(r"KR_ERR_STATE[^;]*layer %zu is MLA", walk) and re.search(r"KR_ERR_STATE[^;]*this store has none", walk)
    # behind every earlier clause, as a caller sees it: the attention-mode bit, the GQA flash-decode options' MLA clause and "multi_mla_fast" speak first
    assert "the attention mode has tolerance bits set" in recorded_refusal("mla/flat", OPT, mode=True)
    assert 'the "multi_attn_fast" option covers GQA layers only' in recorded_refusal("mla/flat", "multi_attn_fast", OPT)
    assert 'the "multi_mla_fast" option covers MLA layers only: this store has none' in recorded_refusal("la/flat", "multi_mla_fast", OPT)
    assert 'the "multi_extend_mla_flash" option covers MLA layers only: this store has none' in recorded_refusal("la/flat", "multi_extend_mla_flash", OPT)
    # its own steps: on an MLA-only store "layer 0 is MLA" comes before "has none"; the geometry rule behind both
    assert recorded_refusal("mla/flat", OPT) == 'RuntimeError: the "multi_extend_flash" option covers GQA layers only: layer 0 is MLA (set the option to 0 for the exact pass)'
    assert recorded_refusal("la/flat", OPT) == 'RuntimeError: the "multi_extend_flash" option covers GQA layers only: this store has none (set the option to 0 for the exact pass)'
    assert recorded_refusal("gqa-3-per-kv/flat", OPT).startswith("ValueError: multi_extend_flash: GQA geometry nh 6 nkv 2 head_dim 64 not covered")
    assert recorded_refusal("la/flat", OPT, "multi_extend_la_chunk") == recorded_refusal("la/flat", OPT)      # ahead of the next rule
    # paged slots under "multi_attn_fast" alone are still refused by the entry points
    assert "if (paged_refused(s))" in _src("kr_decode_multi.cpp") and pre.count("bool paged_refused(") == 1 and pre.count("for (const KrOptRule& r : kr_opt_rules)") == 1      # one predicate, one walker
    assert recorded_refusal("la/paged", "multi_attn_fast", OPT).startswith('RuntimeError: "multi_attn_fast" does not read paged slots')


def test_one_body_two_callers():
    """head_dim 64: one kernel template, instantiated by both callers with their own tile source (as an inlined device function its register allocation
    changed); head_dim 128 / 256: one device function, called by both kernels"""
    dev = _src("kr_pfm_flash_dev.h")
    m = re.search(r"template <([^>]*)>\s*__global__ void __launch_bounds__\(256\) kr_pfm_gqa_flash_kernel\(([^)]*)\)", dev)
    assert m and "class Tiles" in m.group(1) and "typename Tiles::Args a" in m.group(2)
    assert "constexpr bool PAGED = Tiles::PAGED;" in dev
    m = re.search(r"template <([^>]*)>\s*__device__ __forceinline__ void kr_pfm_flashw_body\(([^)]*)\)", dev)
    assert m and "bool PAGED = false" in m.group(1) and "class RowMap" in m.group(1)
    assert "const int* ptab = nullptr" in m.group(2) and "int psh = 0" in m.group(2)
    assert dev.count("if constexpr (PAGED)") >= 6                           # the four-wave form's K and V loads, the wave-specialised form's fast and clamped path
    assert "__builtin_amdgcn_readfirstlane(max(ptab[" in dev                # page ids: clamped, workgroup-uniform, in scalar registers
    assert "__shared__ int" not in dev                                      # no LDS holds the table
    single = _src("kr_attn_flash.hip")
    ahead = single.split("kr_fd_flash_kernel")[0]                           # everything ahead of the decode kernels
    assert "__launch_bounds__(256) kr_pfm_gqa_flash_kernel" not in single   # the four-wave kernel's text is the header's
    assert single.count("kr_pfm_gqa_flash_kernel<H_, F_, KrPfChunkTiles>") == 1 and "struct KrPfChunkTiles" in single
    tiles = single[single.index("struct KrPfChunkTiles"):single.index("};", single.index("struct KrPfChunkTiles"))]
    assert "PAGED = false, SLOTS = false" in tiles and "return t;" in tiles
    calls = re.findall(r"kr_pfm_flashw_body<HD, FP8>\([^;]*;", single)
    assert len(calls) == 1 and "KrPfRowsIdentity()" in calls[0]
    for word in ("slot", "page", "ptab", "pf_tiles", "pf_runs"):
        assert not re.search(r"\b%s" % word, re.sub(r"//.*", "", ahead)), word      # the single-sequence side names no slot and no table
    assert "extern __shared__" not in single                                # the bodies moved whole
    assert "v_max3_f32" not in single and single.count("asm") == 0
    multi = _src("kr_multi_pf_flash.hip")
    m = re.search(r"template <([^>]*)>\s*__global__ void __launch_bounds__\(512, 2\) kr_multi_pf_flashw_kernel\(", multi)
    assert m and "bool PAGED" in m.group(1)
    m = re.search(r"template <([^>]*)>\s*struct KrPfSlotTiles", multi)
    assert m and "bool PAGED_" in m.group(1) and "static constexpr bool PAGED = PAGED_" in multi
    assert "kr_pfm_gqa_flash_kernel<H_, F_, KrPfSlotTiles<F_, true>>" in multi and "kr_pfm_gqa_flash_kernel<H_, F_, KrPfSlotTiles<F_, false>>" in multi
    assert "__launch_bounds__(256)" not in multi                            # no four-wave kernel of its own
    assert "kr_pfm_flashw_body<HD, FP8, true>(" in multi and "kr_pfm_flashw_body<HD, FP8>(" in multi
    assert multi.count("a.page_table + (size_t)slot * a.page_stride") == 2
    assert "kr_m_run_row(i, off, cnt, t)" in multi and "kr_m_run_row(run, off, C, t)" in multi      # the flatten of 17-multi-extend.md
    assert "asm" not in re.sub(r"//.*", "", multi)                          # no inline assembly beyond what the moved bodies hold
    # the form is chosen by the single-sequence launcher's rule
    assert "if (a.hd >= 128)" in single and re.search(r"hd >= 128 \? kr_pfm_flashw_lds\(hd\) : kr_pfm_flash_lds\(hd\)", multi)
    mk = _src("Makefile")
    assert "kr_multi_pf_flash.hip" in mk and "kr_pfm_flash_dev.h" in mk and "kr_pf_tiles.h" in mk


def test_the_batched_launcher_keeps_its_lines_and_gains_the_run_path():
    multi = _src("kr_multi.hip")
    fd = multi[multi.index("if (a.fd_o) {"):multi.index("if (lds > KR_MULTI_GQA_LDS_MAX)")]
    assert "kr_multi_gqa_prep_kernel<true>" in fd and "kr_multi_gqa_prep_kernel<false>" in fd and "return kr_launch_multi_fd(" in fd
    assert multi.index("if (a.pf_tiles) return multi_gqa_runs(a, B, lds, st);") < multi.index("if (a.fd_o) {")
    runs = multi[multi.index("static int multi_gqa_runs(const KrMultiGqaArgs& a, int B, size_t lds, hipStream_t st) {"):]
    assert "dim3(a.nh + a.nkv, B)" in runs                                  # the prep launch over all rows
    assert runs.index("kr_multi_pf_args_ok(a)") < runs.index("kr_multi_gqa_prep_kernel") and runs.index("lds > KR_MULTI_GQA_LDS_MAX") < runs.index("kr_multi_gqa_prep_kernel")      # every check ahead of the first launch
    assert "kr_launch_multi_fd(a, a.pf_nruns, a.fd_chunks, st)" in runs and "dim3(a.nkv, a.pf_nruns)" in runs      # the per-row kernels over the first rows only
    assert "return kr_launch_multi_pf_flash(a, st);" in runs
    # the three per-row kernels leave a row of a longer run at once, ahead of their first barrier
    attn = multi[multi.index("kr_multi_gqa_attn_kernel(const KrMultiGqaArgs a)"):]
    assert attn.index("if (kr_m_row_in_run(a, row)) return;") < attn.index("__syncthreads()")
    flash = _src("kr_multi_flash.hip")
    assert flash.count("if (kr_m_row_in_run(a, b)) return;") == 2
    hdr = _src("kr_multi.h")
    body = re.search(r"struct KrMultiGqaArgs \{(.*?)\n\};", hdr, re.S).group(1)
    assert "const int* page_table; int page_stride, page_shift;" in body
    assert body.rstrip().endswith("const int* pf_runs; const int* pf_tiles; int pf_nruns, pf_ntiles, pf_units;")      # new fields at the end
    assert "return a.pf_runs && a.pf_runs[3 * b + 2] >= 2;" in hdr          # null pointer: no row is skipped
    pre = _src("kr_decode_prefill.cpp")
    plan = _src("kr_multi_plan.h")      # the pass's decisions are the plan's (docs/design/32-multi-pass-plan.md): its check program's cases stand for the lines once pinned here
    assert "o.attn_fast = s->mopt.attn_fast || s->mopt.attn_fast_paged;" in pre and "o.attn_fast && has_gqa && o.max_seq > o.gqa_split_min" in plan
    assert "o.opt = s->mopt;" in pre and "o.opt.extend_flash ? KR_MP_RUNS_FLASH" in plan and case_passed("F")      # never in a verify pass
    assert case_passed("A") and case_passed("B")                             # scratch of the per-row kernels sized by the unit rows
    assert "plan.need_scores && M.scores.ensure(plan.score_bytes)" in pre and "p.score_bytes = (size_t)p.attn_rows * nh_max * p.sc_ld * 4;" in plan and case_passed("K")


def test_the_tile_builder_is_host_only():
    src = _src("kr_pf_tiles.h")
    code = re.sub(r"//.*", "", src)
    assert "hip" not in code.lower() and "__device__" not in code
    assert '#include "kr_pf_tiles.h"' in _src("kr_multi_plan.h") and '#include "kr_multi_plan.h"' in _src("kr_decode_prefill.cpp")


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
    assert not [n for n in exported if "extend_flash" in n or "pf_flash" in n or "pf_tiles" in n]


def test_tile_table_program_under_sanitizers(tmp_path):
    """tiles cover every token of every run of >= 2 exactly once and no token of a unit run, the row map is the flatten, kv_end per tile, counts that are no
    multiples of the tile, 256 runs, T = 1024: tests/pf_tiles_check.cpp with its own main, compiled alone with -fsanitize=address,undefined and run as a child
    process (nothing sanitized is loaded into Python)"""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "pf_tiles_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",
                           "-I", CSRC, "-o", exe, os.path.join(ROOT, "tests", "pf_tiles_check.cpp")])      # runtimes inside the program: no library order to get wrong
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert run.returncode == 0 and "pf tiles ok" in run.stdout, run.stdout
