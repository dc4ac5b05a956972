"""KR_DECODE_FAST launch by launch on ONE-LAYER models: every value the store lets a test read after a step ("tap") against the float64 model of the layer
(tests/decode_f64.py), held to a bound that comes from the reference's own summation error -- not to the 2e-3 of the whole-model tests, inside which a sum that
skips an element, repeats a partial or misses a position fits.

Per case (decode_f64.CASES: proved on the CPU by tests/test_decode_stages.py) the same tokens and positions run from the same reset state (set before EVERY
token, so each step is one layer on inputs that are bit-identical in both modes) in exact mode and under decode_fast=True, graph on; the first LA and the first GQA
case also eagerly; GQA short-cache cases also with "gqa_fused" 0, one MLP case with "lm_fused" 0.  Then per tap, errors against float64, worst over the tokens:

    e_fast <= max(4 * max(e_exact, e_tree), floor)

e_exact: the exact GPU run, which is asserted bit-equal to the oracle on every tap it exposes.  e_tree: the float64 model's code with f32 pairwise sums.  floor: four
units in the last place of the tap's storage type at its largest magnitude (f32; f16 / E4M3 for cache rows).  4 = two bits of room (the kernels' trees are not
numpy's pairwise tree; INT16 / bf16 digit flips are discrete), not tuned to the kernels.  Router ids are equal to the float64 model's on every counted token
(decode_f64.router_gap_ok).  If the mode refuses a geometry the layer runs the exact kernels: then the taps are asserted bit-equal (recorded from profile_step).

WHICH BUFFER HOLDS WHICH SUM (kr_decode.cpp, enqueue_step; kr_decode_read_buffer 0 hidden, 1 residual, 5 second residual, 4 / 2 / 3 router, 6 logits):
  exact step, MoE layer   the input norm writes the residual (= embedding row) to 1; the fused router launch writes residual + attention branch to 5; the down +
                          combine launch leaves the MoE output in 0; the final norm launch writes 5 + 0 to 1 and the normalised vector to 0.
                          After the step: 5 = resid_attn, 1 = resid_final, 0 = normed.  moe_out is overwritten: not readable.
  exact step, dense MLP   the post-attention norm works in place on 1: after the step 1 = resid_final, 0 = normed; resid_attn and moe_out are not readable.
  FAST step               K1 writes the residual to 5; the router launch (or the dense gate|up launch) writes 5 + attention branch to 1; the down (+ combine) launch
                          leaves the MLP output in 0; the folded final norm + lm_head launch writes 1 + 0 to 5 and keeps the normalised vector to itself.
                          After the step: 1 = resid_attn, 0 = moe_out, 5 = resid_final; normed is not readable.
  FAST step, "lm_fused" 0 the final norm launch writes 1 + 0 to 1 and the normalised vector to 0: 1 = resid_final, 0 = normed (5 still holds the embedding row).
moe_out has no exact-GPU reading: its e_exact is the oracle's (the exact run equals the oracle on everything that can be read).
Measured values are appended, one "stages:" line each, to the mode's error log (tests/test_decode_fast_gpu.py, _log); the table of
docs/design/07-decode-fast.md is a copy."""

import numpy as np
import pytest

from tests import decode_f64 as M
from tests.test_decode_fast_gpu import _log as _err_log

pytestmark = pytest.mark.gpu
F = np.float32
PK_RMSNORM, PK_MATVEC, PK_LA_RECUR, PK_ROUTE_LOGITS, PK_MOE_W13, PK_LM_HEAD, PK_OUT_PROJ = 1, 2, 4, 7, 9, 12, 15      # PK_* of krasis_amd/csrc/kr_decode_internal.h
FIRST_EAGER = {c["name"] for c in M.CASES if c.get("eager")}


def _log(msg):
    _err_log("stages: " + msg)


def _buf(st, which, n):
    out = np.empty(n, F)
    assert st._lib.kr_decode_read_buffer(st._h, which, out.ctypes.data, n) == 0
    return out


def _read(st, d, orc, pos, layout, fp8):
    """the taps one step left behind; layout: "exact" | "fast" | "fast-lm-two" (module docstring)"""
    L, H, T = orc.layers[0], d["H"], {}
    if L["attn"] == "la":
        cs = np.empty(d["conv_dim"] * 4, F); rs = np.empty(d["nv"] * d["dk"] * d["dv"], F)
        st.get_decode_state(0, None, None, cs, rs)
        T["conv_new"] = cs.reshape(-1, 4)[:, 3].copy(); T["recur"] = rs.reshape(d["nv"], -1)
    else:
        kc = np.empty((d["kv_max"], d["nkv"] * d["hd"]), np.uint8 if fp8 else np.uint16); vc = np.empty_like(kc)
        st.get_decode_state(0, kc, vc, None, None)
        T["k_code"], T["v_code"] = kc[pos].astype(np.uint16), vc[pos].astype(np.uint16)
        T["k_row"], T["v_row"] = M.cache_to_f32(kc[pos], fp8), M.cache_to_f32(vc[pos], fp8)
    dense = L["mlp"] == "dense"
    if layout == "exact":
        T["resid_final"], T["normed"] = _buf(st, 1, H), _buf(st, 0, H)
        if not dense:
            T["resid_attn"] = _buf(st, 5, H)
    elif layout == "fast":
        T["resid_attn"], T["moe_out"], T["resid_final"] = _buf(st, 1, H), _buf(st, 0, H), _buf(st, 5, H)
    else:
        T["resid_final"], T["normed"] = _buf(st, 1, H), _buf(st, 0, H)
    if not dense:
        T["router_logits"], T["router_ids"], T["router_w"] = st.read_router(L["gate"].shape[0], orc.topk)
    T["logits"] = _buf(st, 6, d["V"])
    return T


def _floor(name, ref, fp8):
    """four units in the last place of the tap's storage type at its largest magnitude, relative to that magnitude"""
    mx = float(np.abs(ref).max())
    if name in ("k_row", "v_row"):
        ulp = 2.0 ** (np.floor(np.log2(mx)) - 3) if fp8 else float(np.spacing(np.float16(mx)))
    else:
        ulp = float(np.spacing(F(mx)))
    return 4.0 * ulp / mx


@pytest.mark.parametrize("ci", range(len(M.CASES)), ids=[c["name"] for c in M.CASES])
def test_fast_step_taps_against_float64(ci):
    case = M.CASES[ci]
    st, eng, orc, keep, d = M.build_case(case)
    fp8 = bool(case.get("fp8"))
    if fp8:
        st.set_kv_dtype(True)
    toks = M.tokens(case)
    ref = [M.step(orc, t, p, M.Ref(), fp8) for t, p in toks]
    t64 = [M.step(orc, t, p, M.Num(False), fp8) for t, p in toks]
    ttr = [M.step(orc, t, p, M.Num(True), fp8) for t, p in toks]
    counted = [M.router_gap_ok(b, M.rel_err(a["router_logits"], b["router_logits"]), orc.topk) if "router_ids" in b else False for a, b in zip(ref, t64)]
    worst = lambda runs, name: max(M.rel_err(a[name], b[name]) for a, b in zip(runs, t64))
    e_tree = {n: worst(ttr, n) for n in case["taps"] if n in t64[0]}

    def run(fast, graph=True, gqa_fused=1, lm_fused=1, layout="exact"):
        st.set_use_graph(graph); st.set_attention_mode(False, decode_fast=fast)
        st.set_option("gqa_fused", gqa_fused); st.set_option("lm_fused", lm_fused)
        out, lg = [], np.empty(d["V"], F)
        for t, p in toks:
            d["reset"]()
            st.decode_step(t, p, lg.ctypes.data)
            out.append(_read(st, d, orc, p, layout, fp8))
            assert np.array_equal(out[-1]["logits"].view(np.uint32), lg.view(np.uint32))
        d["reset"]()
        return out, [c for _, c in st.profile_step(*toks[0])]

    exact, cnt_exact = run(False)
    for a, b in zip(exact, ref):      # the exact graph is still the oracle, tap for tap
        for name, v in a.items():
            assert np.array_equal(np.asarray(v).view(np.uint8), np.asarray(b[name], v.dtype).view(np.uint8)), ("exact run differs from the oracle", case["name"], name)
    e_exact = {n: (worst(exact, n) if n in exact[0] else worst(ref, n)) for n in e_tree}

    legs = [("fast", dict())]
    if case.get("two"):
        legs.append(("fast gqa_fused=0", dict(gqa_fused=0)))
    if case.get("lm_two"):
        legs.append(("fast lm_fused=0", dict(lm_fused=0, layout="fast-lm-two")))
    if case["name"] in FIRST_EAGER:
        legs.append(("fast eager", dict(graph=False)))
    for leg, kw in legs:
        kw.setdefault("layout", "fast")
        probe, cnt = run(True, **kw)
        # every norm folded into a launch of the mode (no norm launch but the one "lm_fused" 0 asks for) = no launcher refused.  The out / o projection runs the
        # mode's K-split kernel where the attention launch leaves an INT16 image (head_dim a multiple of 128); at head_dim 64 it is the exact matvec by design
        folded = cnt[PK_RMSNORM] == (1 if kw["layout"] == "fast-lm-two" else 0)
        _log("%-16s %-18s launches by kind %s -> %s, K-split out projection: %d" % (case["name"], leg, cnt, "the mode's launches" if folded else "REFUSED: exact kernels", cnt[PK_OUT_PROJ]))
        if not folded:      # a launcher refused the geometry: the layer ran the exact kernels, whose buffers and bits are the exact step's
            assert cnt == cnt_exact, (cnt, cnt_exact)
            got, _ = run(True, **dict(kw, layout="exact"))
            for a, b in zip(got, exact):
                for name, v in a.items():
                    assert np.array_equal(np.asarray(v).view(np.uint8), np.asarray(b[name]).view(np.uint8)), (case["name"], leg, name)
            continue
        for name in e_tree:
            if name not in probe[0]:
                continue
            e_fast = worst(probe, name)
            floor = max(_floor(name, b[name], fp8) for b in t64)
            bound = max(4.0 * max(e_exact[name], e_tree[name]), floor)
            base = max(e_exact[name], e_tree[name])
            if name in case.get("digit_taps", ()):      # this case's tap alone: one INT16 digit step of silu * up (decode_f64.CASES says why), far under the cap
                bound = max(bound, max(M.digit_step(orc, t, p) / float(np.abs(b[name]).max()) for (t, p), b in zip(toks, t64)))
                assert bound <= M.CAP
            msg = "%-16s %-18s %-14s e_fast %.3e  e_exact %.3e  e_tree %.3e  ratio %s  bound %.3e" % (
                case["name"], leg, name, e_fast, e_exact[name], e_tree[name], ("%.2f" % (e_fast / base)) if base > 0 else "-", bound)
            print(msg); _log(msg)
            assert 4.0 * base <= M.CAP, (name, base)      # tests/test_decode_stages.py asserts this on the CPU: the bound cannot hide a failure
            assert e_fast <= bound, (case["name"], leg, name, e_fast, bound)
        for i, (a, b) in enumerate(zip(probe, t64)):
            assert all(np.isfinite(np.asarray(v, np.float64)).all() for v in a.values())
            if counted[i]:
                assert np.array_equal(a["router_ids"], b["router_ids"]), (case["name"], leg, toks[i], a["router_ids"], b["router_ids"])
            if fp8:      # the E4M3 floor is half the row's largest value: the stored codes themselves may differ from float64's by one step of the element at most
                for c in ("k_code", "v_code"):
                    x, y = a[c].astype(np.int32), b[c].astype(np.int32)
                    assert (np.abs((x & 127) - (y & 127)) <= 1).all() and (((x ^ y) & 128 == 0) | ((x | y) & 126 == 0)).all(), (case["name"], leg, c)
