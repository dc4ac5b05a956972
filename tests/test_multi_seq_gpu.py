"""Exact batched decode of many sequences held in device slots (kr_decode_slots_create / slot_save / slot_load / step_multi / generate_multi):
every row of a multi-sequence step is BIT-IDENTICAL to kr_decode_step on that sequence alone -- logits, greedy id, the KV row it appends, conv and
recurrent state -- whatever other rows share the step, in whatever order, at whatever positions."""
import numpy as np
import pytest

from tests.test_decode_gpu import build
from tests.test_speculative_gpu import CFGS, _same, _snap

pytestmark = pytest.mark.gpu
F = np.float32
U = np.uint32


def _prompt(rng, d, n):
    return [int(x) for x in rng.integers(0, d["V"], n)]


def _start(st, d, prompt):
    """the store's own sequence = prompt (zero state, then the prompt pass; decode_step token by token where the prompt pass refuses the geometry, dv < dk)"""
    st.reset_decode_state(d["kv_max"])
    if prompt and d["dv"] >= d["dk"]:
        st.prefill(prompt, 0)
    else:
        for i, t in enumerate(prompt):
            st.decode_step(t, i)


def _reference(st, d, prompt, first, n_steps):
    """decode_step alone: per step (logits bits, greedy id); then the state snapshot after the steps"""
    _start(st, d, prompt)
    out, tok, pos = [], first, len(prompt)
    for _ in range(n_steps):
        st.decode_step(tok, pos)
        out.append((st.read_logits().view(U).copy(), st.last_token()))
        tok = out[-1][1]; pos += 1
    return out, _snap(st, d, pos)


def _fill_slots(st, d, prompts, slot_lists):
    """slot_lists[i]: the slots that receive sequence i (its prompt pass, saved)"""
    for p, slots in zip(prompts, slot_lists):
        _start(st, d, p)
        for s in slots:
            st.save_slot(s, len(p))


LA4 = dict(kinds=["la", "la", "la", "la"], la_heads=(4, 16))      # linear attention alone, four value heads per key head
DV64 = dict(la_dkdv=(128, 64), la_heads=(2, 2), seed=5)          # dv < dk: the strided qc / kc fills loop twice, the RMS sum runs over 64 values


@pytest.mark.parametrize("cfg", CFGS + [LA4, DV64])
def test_step_multi_equals_decode_step_alone(cfg):
    st, eng, orc, keep, d = build(kv_max=64, **cfg)
    rng = np.random.default_rng(5)
    prompts = [_prompt(rng, d, n) for n in (1, 40, 7, 23, 12)] + [[]]      # the last slot starts at zero state, position 0
    firsts = [int(x) for x in rng.integers(0, d["V"], len(prompts))]
    refs = [_reference(st, d, p, f, 5) for p, f in zip(prompts, firsts)]
    st.create_slots(len(prompts) + 2, 60)
    slots = [3, 0, 6, 2, 5, 1]                                              # slot numbers need not follow the rows
    _fill_slots(st, d, prompts, [[s] for s in slots])
    toks, pos = list(firsts), [len(p) for p in prompts]
    for k in range(4):
        ids, lg = st.step_multi(slots, toks, pos, logits=True)
        for i, (ref, _) in enumerate(refs):
            assert np.array_equal(lg[i].view(U), ref[k][0]), ("logits", k, i)
            assert ids[i] == ref[k][1], ("id", k, i)
        toks = ids; pos = [p + 1 for p in pos]
    for i, (ref, _) in enumerate(refs):
        ref_after4 = _reference(st, d, prompts[i], firsts[i], 4)[1]
        st.reset_decode_state(d["kv_max"])
        st.load_slot(slots[i], pos[i])
        _same(_snap(st, d, pos[i]), ref_after4)
        st.decode_step(toks[i], pos[i])                                     # the store continues the sequence identically
        assert np.array_equal(st.read_logits().view(U), ref[4][0]) and st.last_token() == ref[4][1], i


def test_batch_sizes_and_row_order():
    st, eng, orc, keep, d = build(kv_max=48)
    rng = np.random.default_rng(9)
    n_seq = 64
    prompts = [_prompt(rng, d, int(rng.integers(1, 9))) for _ in range(n_seq)]
    firsts = [int(x) for x in rng.integers(0, d["V"], n_seq)]
    refs = [_reference(st, d, p, f, 1)[0][0] for p, f in zip(prompts, firsts)]
    batches = [1, 31, 32, 33, 64]
    perm = [int(x) for x in rng.permutation(64)]
    groups, base = [], 0
    for B in batches:
        groups.append((list(range(B)), list(range(base, base + B)))); base += B
    groups.append((perm, list(range(base, base + 64)))); base += 64        # the 64 rows again, permuted
    st.create_slots(base, 48)
    per_seq = [[] for _ in range(n_seq)]
    for seqs, slots in groups:
        for q, s in zip(seqs, slots):
            per_seq[q].append(s)
    _fill_slots(st, d, prompts, per_seq)
    for seqs, slots in groups:
        ids, lg = st.step_multi(slots, [firsts[q] for q in seqs], [len(prompts[q]) for q in seqs], logits=True)
        for r, q in enumerate(seqs):
            assert np.array_equal(lg[r].view(U), refs[q][0]), (len(seqs), r, q)
            assert ids[r] == refs[q][1], (len(seqs), r, q)


@pytest.mark.parametrize("hd,nh,fp8", [(256, 16, False), (256, 16, True), (128, 8, False), (64, 4, False)])
def test_long_caches(hd, nh, fp8):
    """rows below 1024, between 1024 and 4096 and above 4096 positions in one step; the slots' capacity differs from the store's kv_max_seq"""
    kv_max = 4300
    st, eng, orc, keep, d = build(seed=3, hd=hd, nh=nh, kv_max=kv_max)
    if fp8:
        st.set_kv_dtype(True); d["fp8"] = True
    rng = np.random.default_rng(hd)
    prompts = [_prompt(rng, d, n) for n in (700, 2500, 4150)]
    firsts = [int(x) for x in rng.integers(0, d["V"], 3)]
    refs = [_reference(st, d, p, f, 2) for p, f in zip(prompts, firsts)]
    st.create_slots(3, 4400)
    slots = [2, 0, 1]
    _fill_slots(st, d, prompts, [[s] for s in slots])
    toks, pos = list(firsts), [len(p) for p in prompts]
    for k in range(2):
        ids, lg = st.step_multi(slots, toks, pos, logits=True)
        for i, (ref, _) in enumerate(refs):
            assert np.array_equal(lg[i].view(U), ref[k][0]), ("logits", k, i)
            assert ids[i] == ref[k][1], ("id", k, i)
        toks = ids; pos = [p + 1 for p in pos]
    for i, (_, snap) in enumerate(refs):
        st.reset_decode_state(kv_max)
        st.load_slot(slots[i], pos[i])
        _same(_snap(st, d, pos[i]), snap)


def test_generate_multi_equals_generate_greedy():
    st, eng, orc, keep, d = build(kv_max=64)
    rng = np.random.default_rng(13)
    prompts = [_prompt(rng, d, n) for n in (5, 17, 2, 30)]
    firsts = [int(x) for x in rng.integers(0, d["V"], 4)]
    max_tokens = 9
    free = []
    for p, f in zip(prompts, firsts):
        _start(st, d, p); free.append(st.generate_batch(f, len(p), max_tokens))
    stop_ids = [free[0][2], free[2][5]]                                     # rows end at different steps; rows without them reach max_tokens
    ref_toks, ref_snaps = [], []
    for p, f in zip(prompts, firsts):
        _start(st, d, p)
        T = st.generate_batch(f, len(p), max_tokens, stop_ids=stop_ids)
        ref_toks.append(T); ref_snaps.append(_snap(st, d, len(p) + len(T)))
    assert len({len(T) for T in ref_toks}) > 1 and max(len(T) for T in ref_toks) == max_tokens
    st.create_slots(4, 64)
    slots = [1, 3, 0, 2]
    _fill_slots(st, d, prompts, [[s] for s in slots])
    out = st.generate_multi(slots, firsts, [len(p) for p in prompts], max_tokens, stop_ids)
    assert out == ref_toks
    for i, p in enumerate(prompts):
        st.reset_decode_state(d["kv_max"])
        st.load_slot(slots[i], len(p) + len(out[i]))
        _same(_snap(st, d, len(p) + len(out[i])), ref_snaps[i])


@pytest.mark.parametrize("graph", [True, False])
def test_steps_leave_the_store_sequence_alone(graph):
    st, eng, orc, keep, d = build(kv_max=48)
    st.set_use_graph(graph)
    rng = np.random.default_rng(17)
    prompt = _prompt(rng, d, 6)
    toks = _prompt(rng, d, 5)
    ref, _ = _reference(st, d, prompt, toks[0], 5)
    st.create_slots(3, 48)
    _fill_slots(st, d, [_prompt(rng, d, 3), _prompt(rng, d, 9)], [[0], [2]])
    _start(st, d, prompt)
    tok, pos, mpos = toks[0], len(prompt), [3, 9]
    for k in range(5):
        st.decode_step(tok, pos)
        mpos_ids = st.step_multi([2, 0], [toks[k], toks[-1 - k]], [mpos[1], mpos[0]])
        assert len(mpos_ids) == 2
        mpos = [p + 1 for p in mpos]
        assert np.array_equal(st.read_logits().view(U), ref[k][0]) and st.last_token() == ref[k][1], k
        tok = st.last_token(); pos += 1


def test_save_load_round_trip():
    st, eng, orc, keep, d = build(kv_max=40)
    st.fill_state_synthetic(d["kv_max"], seed=3)
    want = _snap(st, d, 29)
    st.create_slots(2, 36)
    st.save_slot(1, 29)
    st.reset_decode_state(d["kv_max"])
    st.load_slot(1, 29)
    _same(_snap(st, d, 29), want)


def test_refusals_change_nothing():
    st, eng, orc, keep, d = build(kv_max=32)
    with pytest.raises(Exception):
        st.step_multi([0], [1], [0])                                       # no slots yet
    st.create_slots(3, 24)
    st.fill_state_synthetic(d["kv_max"], seed=5)
    st.save_slot(1, 20)
    want = _snap(st, d, 20)

    def unchanged():
        st.reset_decode_state(d["kv_max"]); st.load_slot(1, 20)
        _same(_snap(st, d, 20), want)

    V = d["V"]
    bad_steps = [([1, 1], [2, 3], [20, 20]),      # a slot named twice
                 ([3], [2], [20]), ([-1], [2], [20]),   # slot out of range
                 ([1], [V], [20]), ([1], [-1], [20]),   # token out of range
                 ([1], [2], [24]), ([1], [2], [-1]),    # position outside the slot
                 ([], [], []), (list(range(3)) * 86, [0] * 258, [0] * 258)]   # n outside [1, KR_MULTI_MAX]
    for sl, tk, ps in bad_steps:
        with pytest.raises(Exception):
            st.step_multi(sl, tk, ps)
    unchanged()
    for fast in [dict(fast=True), dict(fast=False, gemm_fast=True), dict(fast=False, decode_fast=True)]:
        st.set_attention_mode(**fast)
        with pytest.raises(Exception):
            st.step_multi([1], [2], [20])
        with pytest.raises(Exception):
            st.generate_multi([1], [2], [20], 2)
        st.set_attention_mode(False)
    unchanged()
    with pytest.raises(Exception):
        st.generate_multi([1], [2], [20], 5)                               # 20 + 5 > slot max_seq 24, refused before the first step
    unchanged()
    for n in (-1, 25, 33):
        with pytest.raises(Exception):
            st.save_slot(1, n)
        with pytest.raises(Exception):
            st.load_slot(1, n)
    with pytest.raises(Exception):
        st.save_slot(3, 4)
    st.verify([1, 2], 3)                                                   # a pending verify refuses the steps and the slot copies
    for call in (lambda: st.step_multi([1], [2], [20]), lambda: st.save_slot(1, 4), lambda: st.load_slot(1, 4)):
        with pytest.raises(Exception):
            call()
    st.commit(1)
    unchanged()
    st.set_kv_dtype(True)                                                  # slots hold FP16 rows, the store now E4M3
    st.reset_decode_state(d["kv_max"])
    with pytest.raises(Exception):
        st.step_multi([1], [2], [20])
    with pytest.raises(Exception):
        st.load_slot(1, 20)
    st.set_kv_dtype(False)
    unchanged()
    st.create_slots(2, 40)                                                 # past the rope table (kv_max)
    with pytest.raises(Exception):
        st.step_multi([0], [2], [d["kv_max"]])


def test_production_widths():
    """QCN widths: hidden 2048, top-10 of 72, head_dim 256, 16 query heads on 2 KV heads"""
    st, eng, orc, keep, d = build(seed=23, dims=(2048, 512, 72, 10, 512, 512), hd=256, nh=16, kv_max=160, kinds=["la", "gqa"])
    rng = np.random.default_rng(2)
    prompts = [_prompt(rng, d, n) for n in (90, 3, 41)]
    firsts = [int(x) for x in rng.integers(0, d["V"], 3)]
    refs = [_reference(st, d, p, f, 2) for p, f in zip(prompts, firsts)]
    st.create_slots(3, 150)
    _fill_slots(st, d, prompts, [[0], [1], [2]])
    toks, pos = list(firsts), [len(p) for p in prompts]
    for k in range(2):
        ids, lg = st.step_multi([0, 1, 2], toks, pos, logits=True)
        for i, (ref, _) in enumerate(refs):
            assert np.array_equal(lg[i].view(U), ref[k][0]), ("logits", k, i)
            assert ids[i] == ref[k][1]
        toks = ids; pos = [p + 1 for p in pos]
    for i, (_, snap) in enumerate(refs):
        st.reset_decode_state(d["kv_max"])
        st.load_slot(i, pos[i])
        _same(_snap(st, d, pos[i]), snap)
