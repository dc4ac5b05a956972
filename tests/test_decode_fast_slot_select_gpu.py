"""KR_DECODE_FAST, lean routing rule (softmax scoring, no score correction, renormalised weights): the gate|up launch with "slot_select" 1 -- every routed
workgroup selects the expert id of its own rank only (kr_f_slot_select), an extra grid row publishes the routing -- against "slot_select" 0, the launch in
which every workgroup runs the full top-k select and workgroup (0, 0) publishes (krasis_amd/csrc/kr_decode_fast.hip, docs/design/33-slot-select.md).

Both forms compute the same ids, so everything is compared with array_equal: logits of every step, conv / recurrent state and KV rows after the last
step, greedy tokens, published ids and weights.  The published ids are also held against the oracle's topk_indices on the same logits.  Tie cases are
built with duplicated gate rows (equal logits, bit for bit); each case asserts that its situation occurred in the run."""
import numpy as np
import pytest

from oracle import oracle as O
from tests.test_decode_gpu import build

pytestmark = pytest.mark.gpu
F = np.float32
N_TOK = 64          # steps per run: 32 fed from a fixed random stream (varied routing), then 32 greedy
N_TIE = 128         # tie cases: every token from the random stream, so that each situation turns up


def _states(st, d):
    out = []
    for li, kind in enumerate(d["kinds"]):
        if kind == "la":
            cs = np.empty(d["conv_dim"] * 4, F); rs = np.empty(d["nv"] * d["dk"] * d["dv"], F)
            st.get_decode_state(li, None, None, cs, rs); out += [cs, rs]
        else:
            kc = np.empty((d["kv_max"], d["nkv"] * d["hd"]), np.uint16); vc = np.empty_like(kc)
            st.get_decode_state(li, kc, vc, None, None); out += [kc, vc]
    return out


def _run(st, d, E, k, opt, n_tok=N_TOK, seed=11, greedy=True):
    """n_tok steps from the initial state under "slot_select" = opt -> per step (token fed, logits, router logits, ids, weights), final state"""
    st.set_option("slot_select", opt)
    d["reset"]()
    rng = np.random.default_rng(seed)
    fed = rng.integers(0, d["V"], n_tok)
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


def _assert_same(on, off, E, k, scoring=1, esc=None, oracle_ids=True):
    (s1, st1), (s0, st0) = on, off
    for i, ((t1, l1, r1, i1, w1), (t0, l0, r0, i0, w0)) in enumerate(zip(s1, s0)):
        assert t1 == t0, (i, t1, t0)                                     # greedy tokens (the fed half trivially)
        assert np.array_equal(l1.view(np.uint32), l0.view(np.uint32)), i
        assert np.array_equal(r1.view(np.uint32), r0.view(np.uint32)), i
        assert np.array_equal(i1, i0), (i, i1, i0)
        assert np.array_equal(w1.view(np.uint32), w0.view(np.uint32)), (i, w1, w0)
        if oracle_ids:
            rid = np.asarray(O.route_score_topk(r1, k, scoring, True, esc)[0], np.int32)
            assert np.array_equal(rid, i1), (i, rid, i1)
    for a, b in zip(st1, st0):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))


def _model(E, k, seed, kinds=("la", "gqa"), n_tok=N_TOK, **kw):
    st, eng, orc, keep, d = build(dims=(256, 512, E, k, 128, 128), kinds=list(kinds), kv_max=5 + n_tok + 3, seed=seed, **kw)
    st.set_attention_mode(False, decode_fast=True)
    return st, eng, orc, keep, d


LEAN = [(E, k) for E in (8, 64, 96, 128, 512) for k in (1, 2, 8, 10) if k < E]


@pytest.mark.parametrize("E,k", LEAN)
def test_slot_select_lean_rule_bit_equal(E, k):
    """1 / 2 / 8 keys per lane (E <= 64 / 128 / 512), padded lanes (E = 8, 96), k = 1 (slot 0 is also the last slot) up to k = 10"""
    st, eng, orc, keep, d = _model(E, k, seed=100 + E + k)
    on = _run(st, d, E, k, 1)
    off = _run(st, d, E, k, 0)
    _assert_same(on, off, E, k)


def _paired_gate(gate, E):
    """duplicated rows, disjoint pairs: every other pair sits in ONE lane of the select (neighbours 2j, 2j + 1), the others in two lanes (2j, E / 2 + 2j).
    Few enough pairs that a step without a tie among the leaders is common too (2 / 12 / 24 pairs at E = 16 / 128 / 512)"""
    g = gate.copy()
    for j in range({16: 2, 128: 12, 512: 24}[E]):
        a = 2 * j
        b = a + 1 if j % 2 == 0 else E // 2 + a
        g[b] = g[a]
    return g


def _triple_gate(gate, E):
    g = gate.copy()
    for j in range(max(E // 8, 1)):
        a = 4 * j
        g[a + 1] = g[a]; g[E // 2 + a] = g[a]      # two in one lane (or neighbours), the third elsewhere
    return g


def _sorted_desc(rl):
    return np.sort(rl)[::-1]


TIE_SITUATIONS = {
    "ranks (0, 1)": lambda v, k: v[0] == v[1],
    "ranks (s, s + 1), middle": lambda v, k: any(v[s] == v[s + 1] for s in range(1, k - 1)),
    "ranks (k - 1, k)": lambda v, k: v[k - 1] == v[k],
    "outside the leading k + 1 only": lambda v, k: not np.any(v[:k] == v[1:k + 1]) and bool(np.any(v[k + 1:-1] == v[k + 2:])),
}


@pytest.mark.parametrize("E,k", [(16, 4), (128, 8), (512, 10)])
def test_slot_select_ties_pairs(E, k):
    """equal values at ranks (0, 1), at a middle (s, s + 1), at the (k - 1, k) boundary, and wholly outside the leading k + 1: the tied ranks take the full
    select (heap order), every other rank its own id -- the launch equals the all-full-select launch bit for bit in each situation"""
    st, eng, orc, keep, d = _model(E, k, seed=7 + E, kinds=("gqa",), n_tok=N_TIE)
    eng.set_route_weight_f32(0, _paired_gate(orc.layers[0]["gate"], E), None, None)
    on = _run(st, d, E, k, 1, n_tok=N_TIE, greedy=False)
    off = _run(st, d, E, k, 0, n_tok=N_TIE, greedy=False)
    _assert_same(on, off, E, k)
    seen = {name: sum(bool(f(_sorted_desc(s[2]), k)) for s in on[0]) for name, f in TIE_SITUATIONS.items()}
    print("tie situations seen:", seen)
    assert all(n > 0 for n in seen.values()), seen


@pytest.mark.parametrize("E,k", [(16, 4), (128, 8)])
def test_slot_select_ties_three_way(E, k):
    st, eng, orc, keep, d = _model(E, k, seed=9 + E, kinds=("gqa",), n_tok=N_TIE)
    eng.set_route_weight_f32(0, _triple_gate(orc.layers[0]["gate"], E), None, None)
    on = _run(st, d, E, k, 1, n_tok=N_TIE, greedy=False)
    off = _run(st, d, E, k, 0, n_tok=N_TIE, greedy=False)
    _assert_same(on, off, E, k)
    seen = sum(bool(np.any((v[:k - 1] == v[1:k]) & (v[1:k] == v[2:k + 1]))) for v in (_sorted_desc(s[2]) for s in on[0]))
    print("three-way ties among the leading k + 1:", seen)
    assert seen > 0


@pytest.mark.parametrize("E,k", [(16, 4), (128, 8), (512, 10)])
def test_slot_select_all_equal_logits(E, k):
    st, eng, orc, keep, d = _model(E, k, seed=13 + E, kinds=("gqa",))
    gate = np.repeat(orc.layers[0]["gate"][:1], E, axis=0)
    eng.set_route_weight_f32(0, gate, None, None)
    on = _run(st, d, E, k, 1, n_tok=16)
    off = _run(st, d, E, k, 0, n_tok=16)
    _assert_same(on, off, E, k)
    assert all(np.all(s[2] == s[2][0]) for s in on[0])


@pytest.mark.parametrize("E,k,bias", [(64, 8, -10.0), (130, 6, 0.0), (60, 4, 0.0), (130, 6, -10.0)])
def test_slot_select_other_inputs(E, k, bias):
    """all-negative logits (a router bias of -10: the keys of negative floats), E no multiple of 64 or of 4 (scalar loads, padded lanes), E < 64"""
    st, eng, orc, keep, d = _model(E, k, seed=17 + E, kinds=("gqa",))
    if bias != 0.0:
        eng.set_route_weight_f32(0, orc.layers[0]["gate"], np.full(E, bias, F), None)
    on = _run(st, d, E, k, 1)
    off = _run(st, d, E, k, 0)
    _assert_same(on, off, E, k)
    if bias != 0.0:
        assert all(np.all(s[2] < 0) for s in on[0])


def test_slot_select_not_taken_by_sigmoid_scoring():
    """sigmoid scoring + score correction keeps the full select on every workgroup and the old grid: the option changes nothing"""
    st, eng, orc, keep, d = build(kinds=["la", "gqa"], scoring=0, norm_bias_one=False, rsf=2.5, kv_max=5 + N_TOK + 3, seed=23)
    st.set_attention_mode(False, decode_fast=True)
    esc = orc.layers[-1].get("esc")
    on = _run(st, d, 16, 4, 1)
    off = _run(st, d, 16, 4, 0)
    _assert_same(on, off, 16, 4, scoring=0, esc=esc)
