"""KR_DECODE_FAST: "slot_rows_late_first" 1 against 0 (krasis_amd/csrc/kr_decode_fast.hip, docs/design/35-launch-stragglers.md).

Under the per-slot select, routed grid row y of the gate|up launch serves slot k - 1 - y (1) or slot y (0).  The option changes no value and nothing reads across
workgroups, so everything is compared with array_equal on the raw words: the logits of every step, the router logits, ids and weights, the greedy tokens, the
hidden and both residual buffers, and every layer's conv / recurrent state and KV rows after the last step.  Each case that relies on a situation asserts that
it occurred in the run."""
import numpy as np
import pytest

from tests.test_decode_gpu import build

pytestmark = pytest.mark.gpu
F = np.float32
N_TOK = 32          # steps per run: 16 fed from a fixed random stream (varied routing), then 16 greedy
N_TIE = 128         # tie case: every token from the random stream, so that the situation turns up
PK_RMSNORM, PK_MOE_COMBINE = 1, 11      # positions in the PK_* enum of krasis_amd/csrc/kr_decode_internal.h (= the kinds listed in include/krasis_hip.h)
OPTION = "slot_rows_late_first"


def _states(st, d):
    out = [st.read_hidden(d["H"])]
    for which in (1, 5):      # the two residual buffers (kr_decode_read_buffer)
        r = np.empty(d["H"], F)
        assert st._lib.kr_decode_read_buffer(st._h, which, r.ctypes.data, d["H"]) == 0
        out.append(r)
    for li, kind in enumerate(d["kinds"]):
        if kind == "la":
            cs = np.empty(d["conv_dim"] * 4, F); rs = np.empty(d["nv"] * d["dk"] * d["dv"], F)
            st.get_decode_state(li, None, None, cs, rs); out += [cs, rs]
        else:
            kc = np.empty((d["kv_max"], d["nkv"] * d["hd"]), np.uint16); vc = np.empty_like(kc)
            st.get_decode_state(li, kc, vc, None, None); out += [kc, vc]
    return out


def _run(st, d, E, k, opt, n_tok=N_TOK, seed=11, greedy=True):
    """n_tok steps from the initial state with the option = opt -> per step (token fed, logits, router logits, ids, weights), final state"""
    st.set_option(OPTION, opt)
    d["reset"]()
    fed = np.random.default_rng(seed).integers(0, d["V"], n_tok)
    steps = []
    tok = int(fed[0])
    lg = np.empty(d["V"], F)
    for i in range(n_tok):
        if not greedy or i < n_tok // 2:
            tok = int(fed[i])
        st.decode_step(tok, 5 + i, lg.ctypes.data)
        rl, ids, w = st.read_router(E, k)
        steps.append((tok, lg.copy(), rl, ids, w))
        tok = int(np.argmax(lg))
    return steps, _states(st, d)


def _assert_same(on, off):
    (s1, st1), (s0, st0) = on, off
    for i, ((t1, l1, r1, i1, w1), (t0, l0, r0, i0, w0)) in enumerate(zip(s1, s0)):
        assert t1 == t0, (i, t1, t0)                                     # greedy tokens (the fed half trivially)
        assert np.array_equal(l1.view(np.uint32), l0.view(np.uint32)), i
        assert np.array_equal(r1.view(np.uint32), r0.view(np.uint32)), i
        assert np.array_equal(i1, i0), (i, i1, i0)
        assert np.array_equal(w1.view(np.uint32), w0.view(np.uint32)), (i, w1, w0)
    assert len(st1) == len(st0)
    for a, b in zip(st1, st0):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _ab(st, d, E, k, **kw):
    on = _run(st, d, E, k, 1, **kw)
    off = _run(st, d, E, k, 0, **kw)
    _assert_same(on, off)
    return on


def _model(H=256, E=16, k=4, I=128, seed=0, kinds=("la", "gqa"), n_tok=N_TOK, **kw):
    st, eng, orc, keep, d = build(dims=(H, 512, E, k, I, 128), kinds=list(kinds), kv_max=5 + n_tok + 3, seed=seed, **kw)
    st.set_attention_mode(False, decode_fast=True)
    return st, eng, orc, keep, d


def _assert_mode_moe_launches(st, d):
    """every MoE layer ran the mode's three launches (router, gate|up, down + combine), none the exact kernels.  With "w2_combine" 0 an exact MoE layer hands
    its un-combined rows to a norm launch (the next layer's, or the final one), and an exact native-GGUF layer adds a combine launch; the mode's own layers leave
    a plain hidden vector, so a step of a model whose projections all fold their norm then counts neither."""
    st.set_option("w2_combine", 0)
    cnt = [c for _, c in st.profile_step(3, 5 + N_TOK)]
    st.set_option("w2_combine", 1)
    assert (cnt[PK_RMSNORM], cnt[PK_MOE_COMBINE]) == (0, 0), cnt


LATE = [(E, k) for E in (8, 64, 512) for k in (1, 2, 10) if k < E]      # (E = 8 has no top-10)


@pytest.mark.parametrize("E,k", LATE)
def test_slot_rows_late_first_bit_equal(E, k):
    """1 / 8 keys per lane, padded lanes (E = 8), k = 1 (the mapping is the identity) up to k = 10"""
    st, eng, orc, keep, d = _model(E=E, k=k, seed=300 + E + k)
    _ab(st, d, E, k)
    _assert_mode_moe_launches(st, d)


def test_slot_rows_late_first_tie_at_the_first_row():
    """duplicated gate rows: steps in which rank k - 1 -- the slot of grid row 0 under the option -- ties a neighbour, so that the reversed row takes the
    full-select fallback, and steps in which rank 0, now the last routed row, does"""
    E, k = 16, 4
    st, eng, orc, keep, d = _model(E=E, k=k, seed=7 + E, kinds=("gqa",), n_tok=N_TIE)
    g = orc.layers[0]["gate"].copy()
    for a, b in ((0, 1), (4, 12), (6, 7), (10, 2)):
        g[b] = g[a]
    eng.set_route_weight_f32(0, g, None, None)
    on = _ab(st, d, E, k, n_tok=N_TIE, greedy=False)
    srt = [np.sort(s[2])[::-1] for s in on[0]]
    last = sum(bool(v[k - 1] == v[k] or v[k - 2] == v[k - 1]) for v in srt)
    first = sum(bool(v[0] == v[1]) for v in srt)
    print("steps with a tie at rank k - 1: %d, at rank 0: %d, of %d" % (last, first, N_TIE))
    assert last > 0 and first > 0, (last, first)


def test_slot_rows_late_first_not_taken_by_sigmoid_scoring():
    """sigmoid scoring + score correction keeps the full select on every workgroup and the old grid: the option changes nothing"""
    st, eng, orc, keep, d = build(kinds=["la", "gqa"], scoring=0, norm_bias_one=False, rsf=2.5, kv_max=5 + N_TOK + 3, seed=23)
    st.set_attention_mode(False, decode_fast=True)
    assert orc.layers[-1].get("esc") is not None
    _ab(st, d, 16, 4)
