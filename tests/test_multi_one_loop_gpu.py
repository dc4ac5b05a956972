"""The edges of the one generation loop over slots (generate_slots, kr_decode_multi.cpp) that its four entry points share: no tokens wanted, no drafting in the
lookup forms, a stop id as the first token a row emits.  Every expectation is exact by construction or comes from another path (set_slot_sampler,
generate_batch, the plain form on twin slots)."""
import functools

import numpy as np
import pytest

from tests.test_decode_gpu import build
from tests.test_speculative_gpu import _same, _snap
from tests.test_multi_extend_gpu import _slot_state, _toks
from tests.test_multi_verify_gpu import _fill
from tests.test_multi_verify_sample_gpu import _smp_same

pytestmark = pytest.mark.gpu
A, B = [2, 0], [1, 3]                                            # the rows' slots and their twins
SMP = dict(temperature=[0.8, 0.0], top_k=[5, 0], top_p=[0.9, 1.0], presence_penalty=[0.0, 1.5], rng_seeds=[0x1234567, 99])      # sampled; penalised greedy
N_TOK = 6


@functools.lru_cache(maxsize=None)
def _model():
    """the store, two prompts and their first tokens: built once; every test fills the slots it uses itself"""
    st, eng, orc, keep, d = build(kv_max=32)
    st.create_slots(4, 32)
    rng = np.random.default_rng(41)
    prompts = [_toks(rng, d, 5), _toks(rng, d, 3)]
    return st, d, (eng, orc, keep), prompts, _toks(rng, d, 2), [len(p) for p in prompts]


def _states(st, d, slots, pos, grown=(0, 0)):
    return [_slot_state(st, d, s, p + g) for s, p, g in zip(slots, pos, grown)]


def _twin_samplers(st, firsts):
    for b, f, *p in zip(B, firsts, *SMP.values()):
        st.set_slot_sampler(b, f, *p)


def test_no_tokens_greedy_touches_nothing():
    st, d, _, prompts, firsts, pos = _model()
    _fill(st, d, prompts, [[a] for a in A])
    before, smp = _states(st, d, A, pos, (1, 1)), [st.slot_sampler_state(a) for a in A]      # with the row a stray step would append
    assert st.generate_multi(A, firsts, pos, 0) == [[], []]
    for x, y in zip(_states(st, d, A, pos, (1, 1)), before):
        _same(x, y)
    for a, s in zip(A, smp):
        _smp_same(st.slot_sampler_state(a), s)


def test_no_tokens_sampled_starts_the_samplers():
    st, d, _, prompts, firsts, pos = _model()
    _fill(st, d, prompts, [[a] for a in A])
    before = _states(st, d, A, pos, (1, 1))
    assert st.generate_multi(A, firsts, pos, 0, **SMP) == [[], []]
    _twin_samplers(st, firsts)
    for a, b, f, seed in zip(A, B, firsts, SMP["rng_seeds"]):
        seen, rng = st.slot_sampler_state(a)
        want = np.zeros_like(seen); want[f >> 5] = 1 << (f & 31)
        assert np.array_equal(seen, want) and rng == seed
        _smp_same((seen, rng), st.slot_sampler_state(b))
    for x, y in zip(_states(st, d, A, pos, (1, 1)), before):
        _same(x, y)


@pytest.mark.parametrize("sampled", [False, True])
def test_lookup_without_drafting_is_the_plain_loop(sampled):
    st, d, _, prompts, firsts, pos = _model()
    smp = SMP if sampled else {}
    lookup = st.generate_multi_lookup_sample if sampled else st.generate_multi_lookup
    _fill(st, d, prompts, [[b] for b in B])
    free = st.generate_multi(B, firsts, pos, N_TOK, **smp)
    stops = (free[0][next(k for k in range(1, N_TOK) if free[0].index(free[0][k]) == k)],) if len(set(free[0])) > 1 else ()      # row 0 ends early where it can
    _fill(st, d, prompts, [[a, b] for a, b in zip(A, B)])
    smp_before = [st.slot_sampler_state(a) for a in A]
    want = st.generate_multi(B, firsts, pos, N_TOK, stop_ids=stops, **smp)
    ctx = [[f] + w for f, w in zip(firsts, free)]                # contexts that would make every draft right
    got = lookup(A, firsts, pos, N_TOK, contexts=ctx, max_draft=0, stop_ids=stops, **smp)
    assert got == want
    grown = [len(w) for w in want]
    for x, y in zip(_states(st, d, A, pos, grown), _states(st, d, B, pos, grown)):
        _same(x, y)
    for a, b, s in zip(A, B, smp_before):                        # the samplers went the twins' way; the greedy form leaves them alone
        _smp_same(st.slot_sampler_state(a), st.slot_sampler_state(b) if sampled else s)
    assert st.last_multi_lookup_stats == {"passes": max(grown), "accepted": [0, 0]}      # a pass per token of the longest row


@pytest.mark.parametrize("form", ["plain", "lookup"])
def test_a_stop_id_as_the_first_token_of_a_row(form):
    st, d, _, prompts, firsts, pos = _model()

    def alone(i, first, stops):
        st.reset_decode_state(d["kv_max"])
        st.prefill(prompts[i], 0)
        T = st.generate_batch(first, pos[i], N_TOK, stop_ids=stops)
        return T, _snap(st, d, pos[i] + len(T))

    stop = alone(0, firsts[0], ())[0][0]
    # row 1 starts with the first token after which it never emits row 0's first one
    firsts = [firsts[0], next(f for f in ((firsts[1] + j) % d["V"] for j in range(16)) if len(alone(1, f, (stop,))[0]) == N_TOK)]
    refs = [alone(i, firsts[i], (stop,)) for i in range(2)]
    assert len(refs[0][0]) == 1 and len(refs[1][0]) == N_TOK
    _fill(st, d, prompts, [[a] for a in A])
    if form == "plain":
        got = st.generate_multi(A, firsts, pos, N_TOK, stop_ids=(stop,))
    else:
        got = st.generate_multi_lookup(A, firsts, pos, N_TOK, contexts=[[firsts[i]] + alone(i, firsts[i], ())[0] for i in range(2)], max_draft=4, stop_ids=(stop,))
    assert got == [T for T, _ in refs]
    for x, (T, snap) in zip(_states(st, d, A, pos, [len(T) for T, _ in refs]), refs):
        _same(x, snap)
