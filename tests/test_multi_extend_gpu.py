"""Multi-token extend of device slots (kr_decode_extend_multi / extend_multi / prefill_slot, docs/design/17-multi-extend.md): a row that consumes a
run of tokens is BIT-IDENTICAL to that many kr_decode_step calls on that sequence alone -- every KV row (MLA: latent and rope-key row) the tokens
append, the conv and recurrent state afterwards, the last token's logits and the id -- however the stream is cut into calls, whatever rows share the
pass, in whatever order, below and above the 32-row switch of the router.  The yardstick everywhere is decode_step, token by token, on the store's own
sequence (under "multi_attn_fast": step_multi with the option on, token by token); u32 bit patterns, no tolerances."""
import numpy as np
import pytest

from krasis_amd._lib import KR_EXTEND_MAX_TOKENS
from tests.test_decode_gpu import build
from tests.test_speculative_gpu import CFGS, _same, _snap
from tests.test_multi_seq_gpu import DV64, LA4
from tests import test_multi_mla_gpu as mla

pytestmark = pytest.mark.gpu
F = np.float32
U = np.uint32

# (tokens already in the slot, tokens of the run): an empty slot with one token; a run that crosses the conv kernel's four carried inputs twice; a
# prompt + run; a plain decode row; a short run on a short prompt
SEQS = [(0, 1), (0, 9), (7, 5), (23, 1), (2, 3)]
SLOTS = [3, 0, 6, 2, 5]                                          # slot numbers do not follow the rows


def _toks(rng, d, n):
    return [int(x) for x in rng.integers(0, d["V"], n)]


def _logits(st):
    return st.read_logits().view(U).copy()


def _reference(st, d, prompt, run, fill=(), snap=_snap, via_prefill=False):
    """decode_step alone from zero state: the prompt (saved into the slots `fill`), then the run -> logits bits and id after its last token, the
    state snapshot, and the (logits, id) of one further step on that id"""
    st.reset_decode_state(d["kv_max"])
    if via_prefill and prompt:
        st.prefill(prompt, 0)
    else:
        for i, t in enumerate(prompt):
            st.decode_step(t, i)
    for s in fill:
        st.save_slot(s, len(prompt))
    pos = len(prompt)
    for t in run:
        st.decode_step(t, pos); pos += 1
    ref = dict(lg=_logits(st), tok=st.last_token(), snap=snap(st, d, pos), pos=pos)
    st.decode_step(ref["tok"], pos)
    ref["next"] = (_logits(st), st.last_token())
    return ref


def _slot_state(st, d, slot, pos, snap=_snap):
    st.reset_decode_state(d["kv_max"])
    st.load_slot(slot, pos)
    return snap(st, d, pos)


def _assert_rows(st, d, refs, slots, ids, lg, same=_same, snap=_snap):
    for i, (ref, s) in enumerate(zip(refs, slots)):
        assert np.array_equal(lg[i].view(U), ref["lg"]), ("logits", i)
        assert ids[i] == ref["tok"], ("id", i)
        same(_slot_state(st, d, s, ref["pos"], snap), ref["snap"])


def _setup(st, d, rng, seqs, slots):
    prompts = [_toks(rng, d, p) for p, _ in seqs]
    runs = [_toks(rng, d, r) for _, r in seqs]
    refs = [_reference(st, d, p, r, [s]) for p, r, s in zip(prompts, runs, slots)]
    return prompts, runs, refs


@pytest.mark.parametrize("cfg", CFGS + [LA4, DV64])
def test_extend_equals_decode_step_alone(cfg):
    st, eng, orc, keep, d = build(kv_max=64, **cfg)
    st.create_slots(8, 60)
    prompts, runs, refs = _setup(st, d, np.random.default_rng(5), SEQS, SLOTS)
    assert sum(len(r) for r in runs) == 19
    ids, lg = st.extend_multi(SLOTS, runs, [len(p) for p in prompts], logits=True)
    _assert_rows(st, d, refs, SLOTS, ids, lg)
    ids2, lg2 = st.step_multi(SLOTS, ids, [r["pos"] for r in refs], logits=True)      # the slots continue as the sequences do
    for i, ref in enumerate(refs):
        assert np.array_equal(lg2[i].view(U), ref["next"][0]) and ids2[i] == ref["next"][1], i


def test_router_forms_and_row_order():
    """T = 39 tokens (the router's 32-row form) with the rows permuted: every row as in the 19-token call"""
    st, eng, orc, keep, d = build(kv_max=64)
    st.create_slots(8, 60)
    seqs, slots = SEQS + [(4, 20)], SLOTS + [7]
    prompts, runs, refs = _setup(st, d, np.random.default_rng(5), seqs, slots)
    assert sum(len(r) for r in runs) == 39
    order = [5, 2, 0, 4, 1, 3]
    pick = lambda xs: [xs[i] for i in order]
    ids, lg = st.extend_multi(pick(slots), pick(runs), pick([len(p) for p in prompts]), logits=True)
    _assert_rows(st, d, pick(refs), pick(slots), ids, lg)


@pytest.mark.parametrize("cfg", [dict(), LA4])
def test_cut_invariance(cfg):
    """one 12-token stream into three copies of a slot: one run of 12 = runs of 5 + 7 = twelve single-token steps = decode_step alone"""
    st, eng, orc, keep, d = build(kv_max=64, **cfg)
    st.create_slots(4, 40)
    rng = np.random.default_rng(11)
    prompt, stream = _toks(rng, d, 6), _toks(rng, d, 12)
    ref = _reference(st, d, prompt, stream, [0, 1, 2])
    p0 = len(prompt)
    a = st.extend_multi([0], [stream], [p0], logits=True)
    st.extend_multi([1], [stream[:5]], [p0])
    b = st.extend_multi([1], [stream[5:]], [p0 + 5], logits=True)
    for k, t in enumerate(stream):
        c = st.step_multi([2], [t], [p0 + k], logits=True)
    for slot, (ids, lg) in enumerate((a, b, c)):
        _assert_rows(st, d, [ref], [slot], ids, lg)


def test_positions_across_1024_e4m3_head_dim_256():
    st, eng, orc, keep, d = build(seed=3, hd=256, nh=16, kv_max=1100)
    st.set_kv_dtype(True); d["fp8"] = True
    st.create_slots(6, 1100)
    rng = np.random.default_rng(256)
    prompts, runs = [_toks(rng, d, 1019), _toks(rng, d, 3)], [_toks(rng, d, 9), _toks(rng, d, 2)]
    # the prompts through the prompt pass (held to decode_step by the prompt-pass tests); the runs by decode_step
    refs = [_reference(st, d, p, r, fill, via_prefill=True) for p, r, fill in zip(prompts, runs, ([0, 2, 4], [1, 3, 5]))]
    pos = [len(p) for p in prompts]
    assert pos[0] + len(runs[0]) - 1 == 1027
    ids, lg = st.extend_multi([0, 1], runs, pos, logits=True)
    _assert_rows(st, d, refs, [0, 1], ids, lg)
    st.set_option("multi_attn_fast", 1)      # slots of max_seq > 1024: every token carries the bits step_multi gives it under the option
    try:
        got = st.extend_multi([2, 3], runs, pos, logits=True)
        for k in range(9):
            live = [i for i in (0, 1) if k < len(runs[i])]
            ids_k, lg_k = st.step_multi([4 + i for i in live], [runs[i][k] for i in live], [pos[i] + k for i in live], logits=True)
            for r, i in enumerate(live):
                if k == len(runs[i]) - 1:
                    assert np.array_equal(got[1][i].view(U), lg_k[r].view(U)), ("fast logits", i)
                    assert got[0][i] == ids_k[r], ("fast id", i)
    finally:
        st.set_option("multi_attn_fast", 0)
    for i in (0, 1):
        end = pos[i] + len(runs[i])
        _same(_slot_state(st, d, 2 + i, end), _slot_state(st, d, 4 + i, end))


@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("cfg", mla.CFGS)
def test_mla(cfg, fp8):
    st, eng, keep, d = mla._build(fp8, kv_max=64, **cfg)
    st.create_slots(4, 60)
    rng = np.random.default_rng(15)
    seqs, slots = [(0, 1), (5, 6), (11, 17)], [2, 0, 3]
    prompts = [_toks(rng, d, p) for p, _ in seqs]
    runs = [_toks(rng, d, r) for _, r in seqs]
    refs = [_reference(st, d, p, r, [s], snap=mla._snap) for p, r, s in zip(prompts, runs, slots)]
    ids, lg = st.extend_multi(slots, runs, [len(p) for p in prompts], logits=True)
    _assert_rows(st, d, refs, slots, ids, lg, same=mla._same, snap=mla._snap)


def test_sampled_row_draws_once_on_the_last_token():
    st, eng, orc, keep, d = build(kv_max=48)
    st.create_slots(2, 40)
    rng = np.random.default_rng(21)
    prompt, run = _toks(rng, d, 4), _toks(rng, d, 5)
    _reference(st, d, prompt, [], [0, 1])
    for s in (0, 1):
        st.set_slot_sampler(s, prompt[-1], 0.8, 20, 0.9, 0.5, 1234567)
    p0 = len(prompt)
    for k in range(4):
        st.step_multi([0], [run[k]], [p0 + k])
    a, lga = st.step_multi_sample([0], [run[4]], [p0 + 4], logits=True)
    b, lgb = st.extend_multi([1], [run], [p0], logits=True, sample=True)
    assert a == b and np.array_equal(lga.view(U), lgb.view(U))
    a2 = st.step_multi_sample([0], a, [p0 + 5])          # RNG state and seen set advanced alike
    b2 = st.step_multi_sample([1], b, [p0 + 5])
    assert a2 == b2


def test_refusals_leave_everything_as_it_was():
    st, eng, orc, keep, d = build(kv_max=32)
    with pytest.raises(RuntimeError, match="no sequence slots"):
        st.extend_multi([0], [[1, 2]], [0])                                 # no slots
    st.create_slots(3, 24)
    st.fill_state_synthetic(d["kv_max"], seed=5)
    st.save_slot(1, 20)
    st.fill_state_synthetic(d["kv_max"], seed=6)
    st.save_slot(2, 10)
    state = lambda: (_slot_state(st, d, 1, 20), _slot_state(st, d, 2, 10))
    want = state()
    V = d["V"]
    refused = [
        (([1, 2], [[3], []], [20, 10]), "row 1"),                                           # a count of 0
        (([1, 2], [[1] * 1000, [1] * (KR_EXTEND_MAX_TOKENS - 999)], [0, 0]), "row 1"),      # KR_EXTEND_MAX_TOKENS + 1 tokens
        (([1, 1], [[3], [4]], [20, 21]), "row 1"),                                          # a slot named twice
        (([2, 1], [[3], [1, 2, 3, 4, 5]], [10, 20]), "row 1"),                              # last position == max_seq
        (([1], [[2, V, 3]], [20]), "row 0"),                                                # a token outside the vocabulary inside a run
    ]
    for args, row in refused:
        with pytest.raises(ValueError, match=row):
            st.extend_multi(*args)
        got = state()
        for g, w in zip(got, want):
            _same(g, w)
    st.set_attention_mode(fast=True)                                                        # a tolerance bit
    try:
        with pytest.raises(RuntimeError, match="exact-mode only"):
            st.extend_multi([1], [[2, 3]], [20])
    finally:
        st.set_attention_mode(False)
    for g, w in zip(state(), want):
        _same(g, w)


def test_prefill_slot_equals_prefill_and_leaves_the_store_alone():
    st, eng, orc, keep, d = build(kv_max=48)
    st.create_slots(2, 40)
    rng = np.random.default_rng(31)
    toks, own = _toks(rng, d, 21), _toks(rng, d, 6)
    st.reset_decode_state(d["kv_max"])
    st.prefill(toks, 0)
    want_id, want = st.last_token(), _snap(st, d, 21)
    st.reset_decode_state(d["kv_max"])
    st.prefill(own, 0)                                                     # the store's own sequence: something else
    before = (_logits(st), st.last_token(), _snap(st, d, 48))
    assert st.prefill_slot(1, toks, chunk=8) == want_id
    after = (_logits(st), st.last_token(), _snap(st, d, 48))
    assert np.array_equal(before[0], after[0]) and before[1] == after[1]
    _same(after[2], before[2])
    _same(_slot_state(st, d, 1, 21), want)
