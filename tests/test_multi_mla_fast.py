"""The "multi_mla_fast" option (docs/design/24-multi-mla-fast.md) at the drop-in boundary, without a GPU: the MLA flash body is one device function with
paging as a template parameter, the single-sequence kernel calls it without a table, the batched chunk kernel is templated on paging and its merge is
not, the launcher dispatches the paged instantiations and raises their LDS window, the option is known to kr_decode_set_option, the headers and the
Python docstrings, and the library exports exactly the symbols it declares."""
import os
import re
import subprocess

from tests.test_multi_pass_plan import case_passed

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "krasis_amd", "csrc")
OPT = "multi_mla_fast"


def _src(name):
    return open(os.path.join(CSRC, name)).read()


def test_paging_is_a_template_parameter_of_the_body_and_the_kernel():
    """compiled in or out: the flat instantiations (and the single-sequence kernel, which names no table) are the code they were"""
    dev = _src("kr_mla_flash_dev.h")
    body = re.search(r"template <([^>]*)>\s*__device__ __forceinline__ void kr_mla_flash_body\(([^)]*)\)", dev)
    assert body and "bool SPLIT" in body.group(1) and "bool PAGED = false" in body.group(1)
    assert "const int* ptab = nullptr" in body.group(2) and "int psh = 0" in body.group(2)
    assert dev.count("if constexpr (PAGED)") >= 2                          # the table entry of the tile, and the cache addresses
    assert "__builtin_amdgcn_readfirstlane(max(ptab[p0 >> psh], 0))" in dev     # one page id per tile: clamped, workgroup-uniform, in scalar registers
    code = re.sub(r"//[^\n]*", "", dev)
    assert "asm(" not in code and "asm volatile" not in code
    assert code.count("ptab") == 2                                          # the parameter and that one read: no LDS copy of the table
    single = _src("kr_mla_flash.hip")
    call = re.search(r"kr_mla_flash_body<KLR, FP8, SPLIT>\([^;]*;", single)
    assert call and "page" not in call.group(0) and "ptab" not in single and "page_table" not in single
    assert "extern __shared__" not in single                                # the body moved whole
    multi = _src("kr_multi_mla_flash.hip")
    kernel = re.search(r"template <([^>]*)>\s*__global__ void __launch_bounds__\(256\) kr_multi_mla_flash_kernel\(", multi)
    assert kernel and "bool PAGED" in kernel.group(1)
    assert "kr_mla_flash_body<KLR, FP8, true, true>(" in multi and "kr_mla_flash_body<KLR, FP8, true>(" in multi
    assert "a.page_table + slot * a.page_stride, a.page_shift" in multi
    merge = re.search(r"template <([^>]*)>\s*__global__ void __launch_bounds__\(1024\) kr_multi_mla_merge_kernel\(([^)]*)\)", multi)
    assert merge and "PAGED" not in merge.group(1) and "page" not in merge.group(2)      # partials are indexed by row, not by slot
    assert "kr_fd_merge2_body<KLR>(a.positions[b] + 1, blockIdx.x," in multi


def test_launcher_dispatches_and_prepares_the_paged_instantiations():
    multi = _src("kr_multi_mla_flash.hip")
    assert re.search(r"if \(a\.page_table\) hipLaunchKernelGGL\(\(kr_multi_mla_flash_kernel<K_, F_, true>\)", multi)
    assert re.search(r"int kr_multi_mla_fd_prepare\(int klr, int fp8, int paged\)", multi)
    assert "kr_lds_optin(paged ? multi_mla_fd_fn<true>(klr, fp8) : multi_mla_fd_fn<false>(klr, fp8), lds)" in multi
    for klr in (512, 256):
        for fp8 in ("true", "false"):
            assert "kr_multi_mla_flash_kernel<%d, %s, PAGED>" % (klr, fp8) in multi
    launch = _src("kr_multi.hip")
    fn = launch[launch.index("int kr_launch_multi_mla(const KrMultiMlaArgs& a_in"):launch.index("// ---- paged slots: freshly mapped pages read as zero")]
    assert "if (a.fd_o) break;" in fn and "kr_launch_multi_mla_fd(a, B, st)" in fn
    assert fn.index("kr_multi_mla_fd_ok(") < fn.index("kr_launch_mla_absorb_mfma(")      # the geometry is checked before the first launch
    assert "kr_launch_mla_wvc_mfma(" in fn and "kr_launch_mla_wvc(m, st, B)" in fn        # the projection after the attention stays
    pre = _src("kr_decode_prefill.cpp")
    assert "kr_multi_mla_fd_prepare(L.klr, M.kv_fp8, M.pg.paged())" in pre and "M.mla_fd_ready" in pre
    assert "kr_mla_flash_decode_chunk(M.max_seq)" in pre
    assert "(has_mla && !mla_flash && p.mla_row_attn)" in _src("kr_multi_plan.h") and case_passed("D")      # no score rows when no layer reads them: the plan's (docs/design/32-multi-pass-plan.md)
    assert "o.mla_chunk = kr_mla_flash_decode_chunk(M.max_seq);" in pre and case_passed("I")
    assert "kr_multi_mla_flash.hip" in _src("Makefile") and "kr_mla_flash_dev.h" in _src("Makefile")


def test_the_option_is_known_everywhere():
    assert '!strcmp(name, "%s")' % OPT in _src("kr_decode.cpp")
    from tests.util import option_field, recorded_refusal, rule_row
    assert option_field(OPT) == "mla_fast"
    pre = _src("kr_decode_prefill.cpp")
    plan = _src("kr_multi_plan.h")
    assert "o.opt.mla_fast && has_mla && o.max_seq > o.mla_split_min" in plan
    # the two GQA options keep their clauses, ahead of the new option's
    assert "o.attn_fast = s->mopt.attn_fast || s->mopt.attn_fast_paged;" in pre
    assert plan.index("o.attn_fast && has_gqa && o.max_seq > o.gqa_split_min") < plan.index("o.opt.mla_fast && has_mla && o.max_seq > o.mla_split_min")
    refuse = pre[pre.index("int kr_exact_refuse("):pre.index("int kr_spec_refuse(")]
    assert refuse.index("slots && (s->mopt.attn_fast || s->mopt.attn_fast_paged)") < refuse.index("does not run under expert parallelism")
    # its rule is the first of the list, which is walked behind every base clause; it alone does not stand back, and its geometry rule is asked ahead of "has none"
    row = rule_row(OPT)
    assert pre.index("int kr_spec_refuse(") < pre.index("static const KrOptRule kr_opt_rules[] = {") < pre.index(row[:40])
    assert row.startswith('{"multi_mla_fast", &KrMultiOpts::mla_fast, ATTN_MLA, false, nullptr, nullptr, nullptr, 0, true, " for the exact step",')
    assert row.count(OPT + ":") + row.count('"%s"' % OPT) >= 2   # both refusals name the option
    # where the order is seen: on an MLA-only store the GQA options' clause speaks ahead of this option's rule; on a store without MLA layers the option
    # refuses, also on paged slots under "multi_attn_fast" alone; the attention-mode bit speaks ahead of it
    assert 'the "multi_attn_fast" option covers GQA layers only: layer 0 is MLA' in recorded_refusal("mla/flat", "multi_attn_fast", OPT)
    none = 'RuntimeError: the "multi_mla_fast" option covers MLA layers only: this store has none (set the option to 0 for the exact step)'
    assert recorded_refusal("gqa/flat", OPT) == none and recorded_refusal("hybrid/paged", "multi_attn_fast", OPT) == none and recorded_refusal("mla/flat", OPT) == "ok"
    assert "the attention mode has tolerance bits set" in recorded_refusal("la/flat", OPT, mode=True)
    header = open(os.path.join(ROOT, "include", "krasis_hip.h")).read()
    assert header.count('"%s"' % OPT) >= 3
    from krasis_amd.decode_store import CpuDecodeStore
    for fn in (CpuDecodeStore.set_option, CpuDecodeStore.step_multi, CpuDecodeStore.create_slots):
        assert OPT in fn.__doc__, fn.__name__
    assert os.path.exists(os.path.join(ROOT, "docs", "design", "24-multi-mla-fast.md"))


def test_library_exports_exactly_the_declared_symbols():
    """no C-ABI symbol was added: the exported kr_* functions are the ones include/krasis_hip.h declares and krasis_amd._lib binds"""
    from krasis_amd import _lib
    if not os.path.exists(_lib.lib_path()):
        subprocess.check_call(["make", "-C", CSRC])
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.lib_path()], stdout=subprocess.PIPE, text=True, check=True).stdout
    exported = {line.split()[-1] for line in out.splitlines() if re.search(r" T kr_\w+$", line)}
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "krasis_hip.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(kr_\w+)\s*\(", header))
    assert exported == declared & exported and not exported - declared, sorted(exported - declared)
    assert set(_lib.SYMBOLS) <= exported
    assert not [n for n in exported if "mla_fast" in n or "mla_flash" in n]
