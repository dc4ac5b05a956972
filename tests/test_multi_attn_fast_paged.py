"""The "multi_attn_fast_paged" option (docs/design/23-multi-attn-fast-paged.md) at the drop-in boundary, without a GPU: paging is a template parameter of
the flash-decode body and of the batched chunk kernel, the launcher dispatches the paged instantiations and raises their LDS window, the option is known
to kr_decode_set_option, the header and the Python docstrings, and the library exports exactly the symbols it exported before."""
import os
import re
import subprocess

from tests.test_multi_pass_plan import case_passed

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "krasis_amd", "csrc")
OPT = "multi_attn_fast_paged"


def _src(name):
    return open(os.path.join(CSRC, name)).read()


def test_paging_is_a_template_parameter_of_the_body_and_the_kernel():
    """compiled in or out: the flat instantiations (and the single-sequence kernel, which names no third argument) are the code they were"""
    body = re.search(r"template <([^>]*)>\s*__device__ __forceinline__ void kr_fd_flash_body\(([^)]*)\)", _src("kr_fd_flash_dev.h"))
    assert body and "bool PAGED = false" in body.group(1)
    assert "const int* ptab = nullptr" in body.group(2) and "int psh = 0" in body.group(2)
    dev = _src("kr_fd_flash_dev.h")
    assert dev.count("if constexpr (PAGED)") >= 4                          # the table walk, and the three cache addresses (K, and V's pair)
    assert "__builtin_amdgcn_readfirstlane(max(ptab[" in dev                # page ids: clamped, workgroup-uniform, in scalar registers
    kernel = re.search(r"template <([^>]*)>\s*__global__ void __launch_bounds__\(256\) kr_multi_fd_flash_kernel\(", _src("kr_multi_flash.hip"))
    assert kernel and "bool PAGED" in kernel.group(1)
    assert "a.page_table + (size_t)a.slots[b] * a.page_stride, a.page_shift" in _src("kr_multi_flash.hip")
    single = _src("kr_attn_flash.hip")
    assert "kr_fd_flash_body<HD, FP8>(" in single and "page" not in re.search(r"kr_fd_flash_body<HD, FP8>\([^;]*;", single).group(0)
    merge = re.search(r"template <([^>]*)>\s*__global__ void __launch_bounds__\(1024\) kr_multi_fd_merge_kernel\(", _src("kr_multi_flash.hip"))
    assert merge and "PAGED" not in merge.group(1)                          # partials are indexed by row, not by slot


def test_launcher_dispatches_and_prepares_the_paged_instantiations():
    flash = _src("kr_multi_flash.hip")
    assert re.search(r"if \(a\.page_table\) hipLaunchKernelGGL\(\(kr_multi_fd_flash_kernel<H_, F_, true>\)", flash)
    assert re.search(r"int kr_multi_fd_prepare\(int hd, int fp8, int paged\)", flash)
    assert "kr_lds_optin(paged ? multi_fd_fn<true>(hd, fp8) : multi_fd_fn<false>(hd, fp8), lds)" in flash
    for hd in (256, 128, 64):
        for fp8 in ("true", "false"):
            assert "kr_multi_fd_flash_kernel<%d, %s, PAGED>" % (hd, fp8) in flash
    multi = _src("kr_multi.hip")
    fd = multi[multi.index("if (a.fd_o) {"):multi.index("if (lds > KR_MULTI_GQA_LDS_MAX)")]
    assert "kr_multi_gqa_prep_kernel<true>" in fd and "kr_multi_gqa_prep_kernel<false>" in fd and "return kr_launch_multi_fd(" in fd
    assert not re.search(r"if \(a\.page_table\) return 1;", fd)            # the early return is gone
    assert "kr_multi_fd_prepare(L.hd, M.kv_fp8, M.pg.paged())" in _src("kr_decode_prefill.cpp")


def test_the_option_is_known_everywhere():
    assert '!strcmp(name, "%s")' % OPT in _src("kr_decode.cpp")
    from tests.util import option_field, recorded_refusal
    assert option_field(OPT) == "attn_fast_paged" and option_field("multi_attn_fast") == "attn_fast"
    pre = _src("kr_decode_prefill.cpp")
    assert "o.attn_fast = s->mopt.attn_fast || s->mopt.attn_fast_paged;" in pre      # either option: one flag of the plan (docs/design/32-multi-pass-plan.md)
    assert "o.attn_fast && has_gqa && o.max_seq > o.gqa_split_min" in _src("kr_multi_plan.h") and case_passed("A") and case_passed("I")
    assert "slots && (s->mopt.attn_fast || s->mopt.attn_fast_paged)" in pre      # the MLA refusal covers either option
    refuse = re.search(r"int paged_refuse\(kr_decode_store\* s\) \{(.*?)\n\}", _src("kr_decode_multi.cpp"), re.S).group(1)
    assert "if (paged_refused(s))" in refuse and "paged slots" in refuse
    assert pre.count("bool paged_refused(") == 1 and pre.count("for (const KrOptRule& r : kr_opt_rules)") == 1      # one predicate, one walker of the rule list
    assert "bool paged_refused(const kr_decode_store* s) { return s->multi && s->multi->pg.paged() && s->mopt.attn_fast && !s->mopt.attn_fast_paged; }" in pre
    # as a caller sees it: either option names itself on an MLA store, the paged one governs when both are set; paged slots refuse "multi_attn_fast" alone
    assert 'the "multi_attn_fast_paged" option covers GQA layers only: layer 0 is MLA' in recorded_refusal("mla/paged", OPT)
    assert 'the "multi_attn_fast_paged" option covers GQA layers only: layer 0 is MLA' in recorded_refusal("mla/flat", "multi_attn_fast", OPT)
    assert recorded_refusal("gqa/paged", "multi_attn_fast").startswith('RuntimeError: "multi_attn_fast" does not read paged slots')
    assert recorded_refusal("gqa/paged", OPT) == "ok" and recorded_refusal("gqa/paged", "multi_attn_fast", OPT) == "ok" and recorded_refusal("gqa/flat", "multi_attn_fast") == "ok"
    header = open(os.path.join(ROOT, "include", "krasis_hip.h")).read()
    assert header.count('"%s"' % OPT) >= 3
    from krasis_amd.decode_store import CpuDecodeStore
    for fn in (CpuDecodeStore.set_option, CpuDecodeStore.step_multi, CpuDecodeStore.create_slots):
        assert OPT in fn.__doc__, fn.__name__
    assert os.path.exists(os.path.join(ROOT, "docs", "design", "23-multi-attn-fast-paged.md"))


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
    assert not [n for n in exported if "paged" in n and n != "kr_decode_slots_create_paged"]

