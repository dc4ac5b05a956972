"""Tolerance-mode decode steps (mode bit KR_DECODE_FAST, krasis_amd/csrc/kr_decode_fast.hip) against the exact decode graph (bit-identical to the
reference's CPU decode, src/decode.rs:2690-3520 -- tests/test_decode_gpu.py) on the same model, state and tokens.

What FAST changes: the ORDER of the f32 sums only (lane / wave / workgroup trees instead of the reference's sequential chains: RMSNorm sum of
squares, per-group scale chains of the matvecs, softmax denominator, the kv / output chains of the gated delta rule, L2 norms) and the launch
structure.  The products are the reference's: INT16 activation digits, exact integer group sums, bf16(w_scale) * a_scale, the poly-5 sigmoid,
libm exp / log for the gates.  STATED TOLERANCES (each asserted below, measured values are appended to gpurun_out/decode_fast_err.txt):
    logits        max |fast - exact| <= 2e-3 * max |exact|      (a last-bit difference of a layer output moves single INT16 digits of the next
                                                                  projection's input by one step; that step is what the logits see)
    state         recurrent / conv state and KV rows written by the steps: <= 2e-3 of the tensor's largest magnitude (fp16 KV rows: 1 ulp of fp16 on top)
    greedy token  unchanged on these models
    router        ids == the oracle's topk_indices on the SAME logits, bit for bit (weights within 2e-6 relative: tree softmax sum, v_exp_f32)"""
import os

import numpy as np
import pytest

from oracle import oracle as O
from tests.test_decode_gpu import MIXED, build

pytestmark = pytest.mark.gpu
F = np.float32


def _log(msg):
    if os.path.isdir("gpurun_out"):
        with open("gpurun_out/decode_fast_err.txt", "a") as f:
            f.write(msg + "\n")


def _run(cfg, fast, toks_pos, graph=True, feed=None):
    st, eng, orc, keep, d = build(**cfg)
    st.set_use_graph(graph)
    st.set_attention_mode(False, decode_fast=fast)
    out = []
    tok = toks_pos[0][0]
    for i, (t0, pos) in enumerate(toks_pos):
        if feed is not None:
            tok = feed[i]
        lg = np.empty(d["V"], F); st.decode_step(tok, pos, lg.ctypes.data)
        out.append((tok, lg.copy()))
        tok = int(np.argmax(lg))
    states = []
    for li, kind in enumerate(d["kinds"]):
        if kind == "la":
            cs = np.empty(d["conv_dim"] * 4, F); rs = np.empty(d["nv"] * d["dk"] * d["dv"], F)
            st.get_decode_state(li, None, None, cs, rs); states.append((cs, rs))
        else:
            kc = np.empty((d["kv_max"], d["nkv"] * d["hd"]), np.uint16); vc = np.empty_like(kc)
            st.get_decode_state(li, kc, vc, None, None); states.append((kc.view(np.float16).astype(F), vc.view(np.float16).astype(F)))
    return out, states, (st, eng, orc, keep, d)


CFGS = [
    dict(),                                                    # la, gqa, la; softmax routing, (1 + w) norms, shared expert with sigmoid gate
    dict(norm_bias_one=False, scoring=0, rsf=2.5),             # sigmoid scoring + correction bias, rsf != 1
    dict(kinds=["la"]), dict(kinds=["gqa"]),                   # one layer each: localises a failure
    dict(kinds=["la", "la", "la", "la"], la_heads=(4, 16)),    # hr = 4
    dict(wbits=8),                                             # INT8-g128 everywhere
    dict(with_dense=True),                                     # dense MLP layer: its post-attention norm folded into the gate | up launch (round 6); the down projection is the exact kernel
    dict(dims=(2048, 1024, 32, 10, 512, 512), kinds=["la", "gqa"], la_heads=(4, 8), hd=256, nh=8, seed=3),   # QCN-like widths (H 2048, I 512, k 10)
    dict(dims=(4096, 512, 128, 8, 256, 256), kinds=["gqa", "gqa"], hd=128, nh=16, seed=4),                   # Qwen3-235B-like widths (H 4096: the widest the kernels take, E 128, k 8)
    MIXED,                                                     # mixed INT4 / INT8 inside every group that shares an activation: those layers fall back to the exact launches
]


@pytest.mark.parametrize("ci", range(len(CFGS)))
@pytest.mark.parametrize("graph", [True, False])
def test_fast_decode_matches_exact_within_tolerance(ci, graph):
    cfg = CFGS[ci]
    if graph is False and ci >= 4 and cfg is not MIXED:      # no earlier configuration has mixed widths: its eager leg runs
        pytest.skip("eager launch order is covered by the first configurations")
    toks_pos = [(7, 5), (0, 6), (0, 7), (0, 8), (0, 9), (0, 10)]
    ex, ex_state, _ = _run(cfg, False, toks_pos, graph)
    fa, fa_state, _ = _run(cfg, True, toks_pos, graph, feed=[t for t, _ in ex])     # both runs are fed the exact run's tokens
    worst = 0.0
    for (te, le), (tf, lf) in zip(ex, fa):
        assert np.isfinite(lf).all()
        worst = max(worst, float(np.abs(le - lf).max() / np.abs(le).max()))
    same_tok = all(int(np.argmax(le)) == int(np.argmax(lf)) for (_, le), (_, lf) in zip(ex, fa))
    sworst = 0.0
    for (a0, a1), (b0, b1) in zip(ex_state, fa_state):
        for x, y in ((a0, b0), (a1, b1)):
            sworst = max(sworst, float(np.abs(x - y).max() / max(np.abs(x).max(), 1e-30)))
    _log(f"cfg {ci} graph={graph}: logits rel {worst:.3e}  state rel {sworst:.3e}  greedy same {same_tok}")
    assert worst <= 2e-3, worst
    assert sworst <= 3e-3, sworst
    assert same_tok


def test_fast_mode_mixed_widths_take_the_exact_launches():
    """MIXED under KR_DECODE_FAST: a group of matrices with two widths cannot run as one launch of the mode, so those pieces must take the exact launches.
    Counted from the model (la, gqa, la with MoE; gqa with the dense MLP), not measured: the stand-alone shared-gate matvec exists only on the exact MoE path,
    once per MoE layer = 3 (the mode's own MoE launches carry the gate row: 0); norm launches = 4 input norms (no folded in-projection: ba / k are INT8) + 1
    post-attention norm of the dense layer (gate INT4, up INT8) = 5, the three MoE layers' norms ride in the exact fused router and the final norm in the lm_head
    launch; the un-mixed model of the same layers runs no norm launch at all"""
    PK_RMSNORM, PK_SHARED_GATE = 1, 14      # positions in the PK_* enum of krasis_amd/csrc/kr_decode_internal.h (= the kinds listed in include/krasis_hip.h)
    counts = {}
    for name, cfg in (("mixed", MIXED), ("int4", dict(MIXED, wbits=4))):
        st, eng, orc, keep, d = build(**cfg)
        st.set_attention_mode(False, decode_fast=True)
        lg = np.empty(d["V"], F)
        st.decode_step(7, 5, lg.ctypes.data)
        counts[name] = [c for _, c in st.profile_step(int(np.argmax(lg)), 6)]
    assert (counts["mixed"][PK_SHARED_GATE], counts["mixed"][PK_RMSNORM]) == (3, 5), counts["mixed"]
    assert (counts["int4"][PK_SHARED_GATE], counts["int4"][PK_RMSNORM]) == (0, 0), counts["int4"]


@pytest.mark.parametrize("scoring", [1, 0])
def test_fast_router_ids_equal_oracle_topk_on_the_same_logits(scoring):
    """ids bit-exact for identical logits: the FAST selection (in the prologue of the gate|up launch) against the oracle's moe_route_score_topk
    (decode.rs:4088-4186 + topk_indices :1495-1535) applied to the logits the FAST router launch produced, over many tokens; includes the
    sigmoid + e_score_correction rule (selection on score + bias, weights from the unbiased score)."""
    cfg = dict(kinds=["gqa"], scoring=scoring, norm_bias_one=scoring == 1, seed=21)
    st, eng, orc, keep, d = build(**cfg)
    st.set_attention_mode(False, decode_fast=True)
    E, k = 16, 4
    esc = orc.layers[0].get("esc")
    rng = np.random.default_rng(1)
    lg = np.empty(d["V"], F)
    n_tok, bad, wworst = (10000 if scoring == 1 else 2000), 0, 0.0      # agreement over >= 10 k synthetic tokens
    for i in range(n_tok):
        st.decode_step(int(rng.integers(0, d["V"])), 5 + (i % 20), lg.ctypes.data)
        logits, ids, w = st.read_router(E, k)
        rid, rw = O.route_score_topk(logits, k, scoring, True, esc)[:2]
        bad += int(not np.array_equal(np.asarray(rid, np.int32), ids))
        wworst = max(wworst, float(np.abs(np.asarray(rw, F) - w).max() / np.abs(rw).max()))
    _log(f"router scoring={scoring}: {n_tok - bad}/{n_tok} tokens with ids identical to the oracle on the same logits, weights rel {wworst:.2e}")
    assert bad == 0
    assert wworst <= 2e-6, wworst


@pytest.mark.parametrize("E,k,scoring", [(128, 8, 1), (130, 6, 1), (256, 8, 0), (60, 4, 1), (512, 10, 1)])
def test_fast_router_other_expert_counts(E, k, scoring):
    """the select's register forms: 2 / 4 / 8 logits per lane (E <= 128 / 256 / 512), expert counts that are not a multiple of 4 (scalar loads, padded
    lanes) or of 64; Qwen3-235B's 128-expert top-8 among them.  ids against the oracle on the same logits, 400 tokens each, and logits against the exact graph."""
    cfg = dict(kinds=["gqa"], scoring=scoring, norm_bias_one=scoring == 1, seed=E, dims=(256, 512, E, k, 128, 128))
    st, eng, orc, keep, d = build(**cfg)
    st.set_attention_mode(False, decode_fast=True)
    esc = orc.layers[0].get("esc")
    rng = np.random.default_rng(E + k)
    lg = np.empty(d["V"], F)
    bad, wworst = 0, 0.0
    for i in range(400):
        st.decode_step(int(rng.integers(0, d["V"])), 5 + (i % 20), lg.ctypes.data)
        logits, ids, w = st.read_router(E, k)
        rid, rw = O.route_score_topk(logits, k, scoring, True, esc)[:2]
        bad += int(not np.array_equal(np.asarray(rid, np.int32), ids))
        wworst = max(wworst, float(np.abs(np.asarray(rw, F) - w).max() / np.abs(rw).max()))
    _log(f"router E={E} k={k} scoring={scoring}: {400 - bad}/400 ids identical, weights rel {wworst:.2e}")
    assert bad == 0 and wworst <= 2e-6, (bad, wworst)
    d["reset"]()
    ref = np.empty(d["V"], F); st.set_attention_mode(False); st.decode_step(7, 5, ref.ctypes.data)
    d["reset"]()
    st.set_attention_mode(False, decode_fast=True); st.decode_step(7, 5, lg.ctypes.data)
    assert float(np.abs(lg - ref).max() / np.abs(ref).max()) <= 2e-3


def test_fast_router_tie_falls_back_to_heap_order():
    """equal logits among the leaders: the reference's heap order (not index order) decides -- decode.rs:1531.  A gate with duplicated rows makes
    pairs of experts tie exactly."""
    from krasis_amd import CpuDecodeStore  # noqa: F401  (import side effect: library present)
    cfg = dict(kinds=["gqa"], seed=5)
    st, eng, orc, keep, d = build(**cfg)
    gate = orc.layers[0]["gate"].copy()
    gate[1] = gate[9]; gate[3] = gate[12]; gate[4] = gate[12]      # ties: (1, 9), (3, 4, 12)
    eng.set_route_weight_f32(0, gate, None, None)
    st.set_attention_mode(False, decode_fast=True)
    lg = np.empty(d["V"], F)
    seen_tie = 0
    for i in range(60):
        st.decode_step(3 + i, 5, lg.ctypes.data)
        logits, ids, w = st.read_router(16, 4)
        rid = np.asarray(O.route_score_topk(logits, 4, 1, True, None)[0], np.int32)
        assert np.array_equal(rid, ids), (i, rid, ids)
        top = np.sort(logits)[::-1][:5]
        seen_tie += int(np.any(top[:-1] == top[1:]))
    assert seen_tie > 0, "no step had a tie among the leaders: the fallback was not exercised"


def test_fast_mode_generate_and_profile_step():
    """generate_batch and the per-kind profile run on the FAST graph; the exact graph comes back bit-exact when the bit is cleared"""
    st, eng, orc, keep, d = build(seed=2)
    st.set_attention_mode(False, decode_fast=True)
    toks = st.generate_batch(7, 5, 6, 0.0, 1, 1.0, [], 0.0)
    assert len(toks) == 6
    prof = st.profile_step(7, 11)
    assert sum(n for _, n in prof) > 0
    st.set_attention_mode(False)
    d["reset"]()
    lg = np.empty(d["V"], F); st.decode_step(7, 5, lg.ctypes.data)
    ref = orc.step(7, 5)
    assert np.array_equal(lg.view(np.uint32), ref.view(np.uint32))


@pytest.mark.parametrize("hd,fp8", [(64, False), (128, False), (256, False), (64, True), (128, True), (256, True)])
def test_fast_gqa_short_cache_one_launch(hd, fp8):
    """KR_DECODE_FAST over a short cache (kv_max_seq <= 1024): prep + attention of a GQA layer in ONE launch (kr_fgqa_kernel: QK-norm trees, RoPE, KV append,
    16 lanes per position in the score pass, one wave per cache row in the p.v pass, request batches of 32 positions).  Positions on both sides of the batch
    boundaries and up to the end of a 300-position cache, FP16 and E4M3 caches, head_dim 64 / 128 / 256: logits within the mode's 2e-3 of the oracle driver (the
    exact reference order), same greedy token; the appended K / V rows are the exact path's rows up to the tolerance of their inputs."""
    st, eng, orc, keep, d = build(seed=5, kv_max=300, hd=hd, kinds=["gqa", "la", "gqa"])
    if fp8:
        st.set_kv_dtype(True); O.set_kv_fp8(True)
    try:
        if fp8:
            rng = np.random.default_rng(5); kv = {}
            for li, kind in enumerate(d["kinds"]):
                if kind == "gqa":
                    kc = O.f32_to_e4m3((rng.standard_normal((d["kv_max"], d["nkv"] * d["hd"])) * 0.5).astype(F)); vc = O.f32_to_e4m3((rng.standard_normal((d["kv_max"], d["nkv"] * d["hd"])) * 0.5).astype(F))
                    kv[li] = (kc, vc); orc.layers[li]["kv_k"] = kc.astype(np.uint16); orc.layers[li]["kv_v"] = vc.astype(np.uint16)
            n = len(d["kinds"]); ptr = lambda a: a.ctypes.data
            st.set_decode_state(5, d["kv_max"], [ptr(kv[i][0]) if i in kv else 0 for i in range(n)], [ptr(kv[i][1]) if i in kv else 0 for i in range(n)],
                                [ptr(x) if x is not None else 0 for x in d["state"]["conv"]], [ptr(x) if x is not None else 0 for x in d["state"]["recur"]])
        st.set_attention_mode(False, decode_fast=True)
        # An E4M3 cache element has three mantissa bits: a last-bit difference of a K / V value (the mode's tree sums upstream) can move it by one step of 6 %, in
        # this launch exactly as in the mode's two-launch form (kr_decode_set_option "gqa_fused" 0: measured beside it below).  Stated bound with E4M3 caches: 5e-3.
        bound = 5e-3 if fp8 else 2e-3
        tok = 11; worst = 0.0; worst_two = 0.0
        for pos in [0, 1, 15, 16, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 299]:
            logits = np.empty(d["V"], F)
            st.decode_step(tok, pos, logits.ctypes.data)
            ref = orc.step(tok, pos)
            err = float(np.abs(logits - ref).max() / np.abs(ref).max()); worst = max(worst, err)
            assert np.isfinite(logits).all() and err <= bound, (pos, err)
            assert int(np.argmax(logits)) == O.sample_greedy(ref), pos
            tok = O.sample_greedy(ref)
        _log("fused short-cache GQA launch hd %d %s: worst logits rel err over 17 positions %.3e" % (hd, "E4M3" if fp8 else "FP16", worst))
        for li, kind in enumerate(d["kinds"]):
            if kind != "gqa":
                continue
            if fp8:
                kc = np.empty((d["kv_max"], d["nkv"] * d["hd"]), np.uint8); vc = np.empty_like(kc)
                st.get_decode_state(li, kc, vc, None, None)
                a = O.e4m3_to_f32(kc) if hasattr(O, "e4m3_to_f32") else None
                if a is not None:
                    b = O.e4m3_to_f32(orc.layers[li]["kv_k"].astype(np.uint8))
                    assert float(np.abs(a[:300] - b[:300]).max()) <= 0.13 * float(np.abs(b[:300]).max())      # one E4M3 step of the largest row value at most
            else:
                kc = np.empty((d["kv_max"], d["nkv"] * d["hd"]), np.uint16); vc = np.empty_like(kc)
                st.get_decode_state(li, kc, vc, None, None)
                a = kc.view(np.float16).astype(F); b = orc.layers[li]["kv_k"].view(np.float16).astype(F)
                assert float(np.abs(a - b).max()) <= 3e-3 * float(np.abs(b).max())
                a = vc.view(np.float16).astype(F); b = orc.layers[li]["kv_v"].view(np.float16).astype(F)
                assert float(np.abs(a - b).max()) <= 3e-3 * float(np.abs(b).max())
    finally:
        O.set_kv_fp8(False)


@pytest.mark.parametrize("fp8", [False, True])
def test_fast_gqa_one_launch_vs_two_launches(fp8):
    """the one-launch short-cache form against the mode's two-launch form (prep with tree norms + the staged exact-order attention) on the same model and tokens:
    logits within 2e-3 of each other with an FP16 cache (another order of the same sums), within the E4M3 bound with an E4M3 cache; same greedy tokens"""
    outs = {}
    for fused in (1, 0):
        st, eng, orc, keep, d = build(seed=5, kv_max=300, hd=256, kinds=["gqa", "la", "gqa"])
        if fp8:
            st.set_kv_dtype(True)
            rng = np.random.default_rng(5); kv = {}
            for li, kind in enumerate(d["kinds"]):
                if kind == "gqa":
                    kv[li] = (O.f32_to_e4m3((rng.standard_normal((d["kv_max"], d["nkv"] * d["hd"])) * 0.5).astype(F)), O.f32_to_e4m3((rng.standard_normal((d["kv_max"], d["nkv"] * d["hd"])) * 0.5).astype(F)))
            n = len(d["kinds"]); ptr = lambda a: a.ctypes.data
            st.set_decode_state(5, d["kv_max"], [ptr(kv[i][0]) if i in kv else 0 for i in range(n)], [ptr(kv[i][1]) if i in kv else 0 for i in range(n)],
                                [ptr(x) if x is not None else 0 for x in d["state"]["conv"]], [ptr(x) if x is not None else 0 for x in d["state"]["recur"]])
        st.set_attention_mode(False, decode_fast=True)
        st.set_option("gqa_fused", fused)
        lg = []
        for i, pos in enumerate([0, 1, 31, 32, 33, 100, 255, 256, 299]):
            out = np.empty(d["V"], F); st.decode_step(3 + 7 * i, pos, out.ctypes.data); lg.append(out)
        outs[fused] = lg
    bound = 5e-3 if fp8 else 2e-3
    for a, b in zip(outs[1], outs[0]):
        assert float(np.abs(a - b).max() / np.abs(b).max()) <= bound
        assert int(np.argmax(a)) == int(np.argmax(b))


def test_fast_final_norm_and_lm_head_one_launch_vs_two():
    """KR_DECODE_FAST ends the step with ONE launch (final add + RMSNorm folded into the vocabulary projection, tree sums) instead of the exact-order
    norm launch + the exact-order vocabulary matvec: logits within 1e-4 of the two-launch form (another order of the same products), same greedy tokens"""
    outs = {}
    for fused in (1, 0):
        st, eng, orc, keep, d = build(seed=11, kinds=["la", "gqa"])
        st.set_attention_mode(False, decode_fast=True)
        st.set_option("lm_fused", fused)
        lg = []
        for i, pos in enumerate([0, 1, 2, 17, 31]):
            out = np.empty(d["V"], F); st.decode_step(5 + 3 * i, pos, out.ctypes.data); lg.append(out)
        outs[fused] = lg
    for a, b in zip(outs[1], outs[0]):
        assert np.isfinite(a).all()
        assert float(np.abs(a - b).max() / np.abs(b).max()) <= 1e-4
        assert int(np.argmax(a)) == int(np.argmax(b))
