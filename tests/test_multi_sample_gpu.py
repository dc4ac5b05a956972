"""Per-row sampling in the batched multi-sequence decode (kr_decode_slot_sampler / step_multi_sample / generate_multi_sample, kr_sample_rows):
every row draws exactly the token kr_decode_generate draws for that sequence alone -- same token, same xorshift64 state, same seen set --
whatever other rows share the step, in whatever order, with whatever parameters (docs/design/14-multi-sampling.md)."""
import ctypes as C

import numpy as np
import pytest

from oracle import oracle as O
from tests.test_decode_gpu import build
from tests.test_multi_seq_gpu import _fill_slots, _prompt, _start
from tests.test_speculative_gpu import CFGS, _same, _snap

pytestmark = pytest.mark.gpu
F = np.float32
U = np.uint32

# (temperature, top_k, top_p, presence_penalty): the server defaults, the edge cases of the select path, the per-row path (k > 4096 or the whole
# vocabulary), plain greedy, greedy with a penalty, penalised sampled rows
ROW_PARAMS = [(0.6, 50, 0.95, 0.0), (1.0, 1, 1.0, 0.0), (0.7, 4096, 0.9, 0.0), (1.3, 4097, 0.8, 0.0), (1.0, 0, 0.9, 0.0),
              (0.0, 0, 1.0, 0.0), (0.0, 0, 1.0, 1.5), (0.6, 50, 0.95, 1.5), (0.9, 20, 0.95, 0.7)]


def _sample_rows(lg, params, seen, states, force_loop=False):
    from krasis_amd import _lib
    lib = _lib.load_library()
    n, V = lg.shape
    col = lambda j, t: np.ascontiguousarray([p[j] for p in params], t)
    T, K, P, PEN = col(0, F), col(1, np.int32), col(2, F), col(3, F)
    rng = np.ascontiguousarray(states, np.uint64)
    out = np.empty(n, np.int32)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = lib.kr_sample_rows(ptr(lg), n, V, ptr(T), ptr(K), ptr(P), ptr(PEN), ptr(seen), ptr(rng), ptr(out), int(force_loop))
    assert rc == 0, lib.kr_last_error()
    return [int(x) for x in out], [int(x) for x in rng]


def _oracle_row(lg, params, seen_mask, state):
    """kr_decode_generate's step for one row: penalty on the seen tokens (f32, in numpy first), then sample_from_logits or the first maximum"""
    T, K, P, PEN = params
    lg = lg.copy()
    if PEN != 0.0:
        lg[seen_mask] -= F(PEN)
    if T > 0:
        return O.sample_from_logits(lg, T, K, P, state)
    return O.sample_greedy(lg), state


@pytest.mark.parametrize("B", [1, 7, 64, 256])
def test_sample_rows_match_the_oracle(B):
    V = 151936
    W = (V + 31) // 32
    rng = np.random.default_rng(B)
    lg = (rng.integers(-200, 200, (B, V)).astype(F) * F(0.125)).astype(F)     # coarse grid: the k-th value is tied across the cut
    for b in range(B):
        lg[b, rng.integers(0, V, 3)] = F(-0.0)                                # signed zeros compare equal (partial_cmp)
    lg[:, 7] = lg.max() + F(1)                                                # top_k = 1 / greedy rows: one clear maximum in some rows...
    lg[::2, 7] = lg[::2, 9] = lg.max()                                        # ...a tie of two maxima in the others (the first id wins)
    params = [ROW_PARAMS[(b * 5 + B) % len(ROW_PARAMS)] for b in range(B)]
    mask = rng.random((B, W * 32)) < 0.02                                     # random seen sets
    mask[:, 7] = rng.random(B) < 0.5
    seen = np.packbits(mask.reshape(B, W, 32), axis=-1, bitorder="little").reshape(B, W * 4).view(U)
    states = [int(x) for x in rng.integers(1, 2**63, B)]
    toks, after = _sample_rows(lg, params, seen, states)
    for b in range(B):
        ref_tok, ref_state = _oracle_row(lg[b], params[b], mask[b, :V], states[b])
        assert (toks[b], after[b]) == (ref_tok, ref_state), (b, params[b])
    assert _sample_rows(lg, params, seen, states, force_loop=True) == (toks, after)


def _gen_params(n):
    P = [(0.6, 50, 0.95, 0.0), (0.0, 0, 1.0, 0.0), (0.9, 10, 0.95, 0.7), (0.0, 0, 1.0, 1.5), (1.3, 0, 0.8, 0.0)]
    seeds = [0x1234567, 0x9E3779B9, 77, 5, 0xABCDEF]
    return [P[i % len(P)] for i in range(n)], [seeds[i % len(seeds)] for i in range(n)]


@pytest.mark.parametrize("cfg", CFGS)
def test_generate_multi_sampled_equals_generate_batch(cfg):
    st, eng, orc, keep, d = build(kv_max=64, **cfg)
    rng = np.random.default_rng(21)
    prompts = [_prompt(rng, d, n) for n in (5, 17, 2, 30, 9)]
    firsts = [int(x) for x in rng.integers(0, d["V"], len(prompts))]
    params, seeds = _gen_params(len(prompts))
    max_tokens = 9

    def alone(i, stop_ids):
        _start(st, d, prompts[i])
        T, K, P, PEN = params[i]
        return st.generate_batch(firsts[i], len(prompts[i]), max_tokens, T, K, P, stop_ids, PEN, rng_seed=seeds[i])

    free = [alone(i, ()) for i in range(len(prompts))]
    stop_ids = [free[0][2], free[2][5]]                                     # rows end at different steps
    ref_toks, ref_snaps = [], []
    for i, p in enumerate(prompts):
        T = alone(i, stop_ids)
        ref_toks.append(T); ref_snaps.append(_snap(st, d, len(p) + len(T)))
    assert len({len(T) for T in ref_toks}) > 1
    slots = [1, 4, 0, 2, 3]
    for loop in (0, 1):
        st.set_option("multi_sample_loop", loop)
        st.create_slots(5, 64)
        _fill_slots(st, d, prompts, [[s] for s in slots])
        out = st.generate_multi(slots, firsts, [len(p) for p in prompts], max_tokens, stop_ids,
                                temperature=[p[0] for p in params], top_k=[p[1] for p in params], top_p=[p[2] for p in params],
                                presence_penalty=[p[3] for p in params], rng_seeds=seeds)
        assert out == ref_toks, loop
        for i, p in enumerate(prompts):
            st.reset_decode_state(d["kv_max"])
            st.load_slot(slots[i], len(p) + len(out[i]))
            _same(_snap(st, d, len(p) + len(out[i])), ref_snaps[i])
    st.set_option("multi_sample_loop", 0)


@pytest.mark.parametrize("loop", [0, 1])
def test_continuous_batching(loop):
    """six requests join at steps 0, 2 and 5 and leave after their own lengths; the rows of every call come in a new order.  Slots 6 + q hold
    copies of the same sequences and run step_multi on the same tokens: the logits and the greedy rows' ids must be its bits."""
    st, eng, orc, keep, d = build(kv_max=64)
    st.set_option("multi_sample_loop", loop)
    rng = np.random.default_rng(33)
    reqs = [(0, 8, (0.6, 50, 0.95, 0.0), 11), (0, 3, (0.0, 0, 1.0, 0.0), 12), (2, 6, (0.9, 10, 0.95, 0.7), 13),
            (2, 4, (0.0, 0, 1.0, 1.5), 14), (5, 5, (1.3, 0, 0.8, 0.0), 15), (5, 3, (1.0, 1, 1.0, 0.0), 16)]
    prompts = [_prompt(rng, d, int(n)) for n in rng.integers(1, 20, len(reqs))]
    firsts = [int(x) for x in rng.integers(0, d["V"], len(reqs))]
    refs = []
    for q, (_, L, (T, K, P, PEN), seed) in enumerate(reqs):
        _start(st, d, prompts[q])
        refs.append(st.generate_batch(firsts[q], len(prompts[q]), L, T, K, P, (), PEN, rng_seed=seed))
    slot_of = [4, 1, 5, 0, 3, 2]
    st.create_slots(12, 64)
    _fill_slots(st, d, prompts, [[slot_of[q], 6 + q] for q in range(len(reqs))])
    got = [[] for _ in reqs]
    tok, pos = list(firsts), [len(p) for p in prompts]
    step = 0
    while any(len(got[q]) < reqs[q][1] for q in range(len(reqs))):
        for q, (join, _, (T, K, P, PEN), seed) in enumerate(reqs):
            if join == step:
                st.set_slot_sampler(slot_of[q], firsts[q], T, K, P, PEN, seed)
        act = [q for q, r in enumerate(reqs) if r[0] <= step and len(got[q]) < r[1]]
        act = [act[i] for i in rng.permutation(len(act))]
        if act:
            ids, lg = st.step_multi_sample([slot_of[q] for q in act], [tok[q] for q in act], [pos[q] for q in act], logits=True)
            gids, glg = st.step_multi([6 + q for q in act], [tok[q] for q in act], [pos[q] for q in act], logits=True)
            assert np.array_equal(lg.view(U), glg.view(U)), step
            for r, q in enumerate(act):
                if reqs[q][2][0] == 0.0 and reqs[q][2][3] == 0.0:
                    assert ids[r] == gids[r], (step, q)
                got[q].append(ids[r]); tok[q] = ids[r]; pos[q] += 1
        step += 1
    assert got == refs
    st.set_option("multi_sample_loop", 0)


def test_steps_leave_the_store_sampler_alone():
    st, eng, orc, keep, d = build(kv_max=48)
    rng = np.random.default_rng(41)
    prompt, others = _prompt(rng, d, 6), [_prompt(rng, d, 4), _prompt(rng, d, 11)]
    tok0, pos = 17, len(prompt)
    smp = dict(temperature=0.6, top_k=50, top_p=0.95, presence_penalty=0.5)

    def run(between):
        _start(st, d, prompt)
        st.decode_step(tok0, pos)
        a = st.sample(**smp, rng_seed=0xC0FFEE, reset_seen=True)
        between()
        st.decode_step(a, pos + 1)
        lg = st.read_logits().view(U).copy()
        return a, lg, st.sample(**smp, rng_seed=0)                         # continues the store's RNG state and seen set

    ref = run(lambda: None)
    st.create_slots(2, 48)
    _fill_slots(st, d, others, [[0], [1]])
    _start(st, d, prompt)

    def multi_steps():
        st.set_slot_sampler(0, 3, 0.6, 50, 0.95, 0.5, 99)
        st.set_slot_sampler(1, 4, 0.9, 0, 0.9, 1.5, 98)
        t, p = [3, 4], [len(o) for o in others]
        for _ in range(3):
            t = st.step_multi_sample([1, 0], t[::-1], p[::-1])[::-1]
            p = [x + 1 for x in p]

    got = run(multi_steps)
    assert got[0] == ref[0] and got[2] == ref[2]
    assert np.array_equal(got[1], ref[1])


def test_refusals_change_nothing():
    st, eng, orc, keep, d = build(kv_max=32)
    with pytest.raises(Exception):
        st.set_slot_sampler(0, 1, 0.6, 50, 0.95)                          # no slots yet
    with pytest.raises(Exception):
        st.step_multi_sample([0], [1], [0])
    st.create_slots(3, 24)
    st.fill_state_synthetic(d["kv_max"], seed=5)
    st.save_slot(1, 20)
    want = _snap(st, d, 20)
    first, seed, smp = 9, 0x5EED, (0.6, 50, 0.95, 0.5)
    st.set_slot_sampler(1, first, *smp, seed)

    def unchanged():
        st.reset_decode_state(d["kv_max"]); st.load_slot(1, 20)
        _same(_snap(st, d, 20), want)

    V = d["V"]
    for bad in (dict(slot=3), dict(slot=-1), dict(slot=1, temperature=-0.5)):
        args = dict(slot=1, first_token=2, temperature=0.7, top_k=5, top_p=0.9, presence_penalty=0.0, rng_seed=1)
        args.update(bad)
        with pytest.raises(Exception):
            st.set_slot_sampler(**args)
    with pytest.raises(Exception):
        st.generate_multi([1], [2], [20], 2, temperature=[-1.0])
    for sl, tk, ps in [([1, 1], [2, 3], [20, 20]), ([3], [2], [20]), ([1], [V], [20]), ([1], [2], [24]), ([], [], [])]:
        with pytest.raises(Exception):
            st.step_multi_sample(sl, tk, ps)
    for fast in [dict(fast=True), dict(fast=False, gemm_fast=True), dict(fast=False, decode_fast=True)]:
        st.set_attention_mode(**fast)
        with pytest.raises(Exception):
            st.step_multi_sample([1], [2], [20])
        with pytest.raises(Exception):
            st.set_slot_sampler(1, 2, 0.7, 5, 0.9)
        with pytest.raises(Exception):
            st.generate_multi([1], [2], [20], 2, temperature=0.7)
        st.set_attention_mode(False)
    st.verify([1, 2], 3)                                                   # a pending verify refuses them too
    for call in (lambda: st.step_multi_sample([1], [2], [20]), lambda: st.set_slot_sampler(1, 2, 0.7, 5, 0.9)):
        with pytest.raises(Exception):
            call()
    st.commit(1)
    unchanged()
    # the slot's sampler is the one set before the refusals: seen = {first}, state = seed
    tok, lg = st.step_multi_sample([1], [2], [20], logits=True)
    mask = np.zeros(V, bool); mask[first] = True
    assert tok[0] == _oracle_row(lg[0], smp, mask, seed)[0]
    # kr_decode_slots_create drops every sampler: a fresh slot samples greedily
    st.create_slots(3, 24)
    st.save_slot(1, 20)
    ids, lg = st.step_multi_sample([1], [2], [20], logits=True)
    assert ids[0] == int(np.argmax(lg[0]))                                 # np.argmax: the first maximum
