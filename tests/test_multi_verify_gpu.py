"""Exact speculative verify and commit over device slots (kr_decode_verify_multi / kr_decode_commit_multi / kr_decode_generate_multi_lookup,
docs/design/18-multi-verify.md): a verify of [sampled token, draft] runs gives the greedy id after every token, and a commit of n_keep tokens leaves each
slot BIT-IDENTICAL to n_keep kr_decode_step calls on that sequence alone -- KV rows (MLA: latent and rope-key rows) below the committed length, conv and
recurrent state -- whatever rows share the call, in whatever order; n_keep = 0 leaves a slot as it was.  The yardstick everywhere is decode_step, token by
token, on the store's own sequence (generate_multi for the loop; under "multi_attn_fast": extend_multi with the option on); u32 bit patterns, no
tolerances.  KV rows at or past the committed length are unspecified and are not compared."""
import numpy as np
import pytest

from krasis_amd._lib import KR_VERIFY_MAX
from tests.test_decode_gpu import build
from tests.test_speculative_gpu import CFGS, _same, _snap
from tests.test_multi_seq_gpu import DV64, LA4
from tests.test_multi_extend_gpu import _slot_state, _toks
from tests import test_multi_mla_gpu as mla

pytestmark = pytest.mark.gpu
F = np.float32
U = np.uint32


def _trace(st, d, prompt, first, n, fill=(), snap=_snap):
    """decode_step alone from zero state: the prompt (saved into the slots `fill`), then n greedy steps from `first`.  toks[k] = the token step k
    consumes (toks[0] = first, toks[k + 1] = the id step k gives), lg[k] = the logits bits after step k, snaps[k] = the state after k steps"""
    st.reset_decode_state(d["kv_max"])
    for i, t in enumerate(prompt):
        st.decode_step(t, i)
    p0 = len(prompt)
    for s in fill:
        st.save_slot(s, p0)
    tr = dict(p0=p0, toks=[first], lg=[], snaps=[snap(st, d, p0)])
    for k in range(n):
        st.decode_step(tr["toks"][k], p0 + k)
        tr["lg"].append(st.read_logits().view(U).copy()); tr["toks"].append(st.last_token()); tr["snaps"].append(snap(st, d, p0 + k + 1))
    return tr


def _right(tr, c):
    """a run of c tokens whose drafts are the true greedy continuation"""
    return list(tr["toks"][:c])


def _wrong_at(tr, c, j, V):
    run = _right(tr, c)
    run[j] = (run[j] + 1) % V
    return run


def _check_slot(st, d, slot, tr, k, snap=_snap, same=_same):
    same(_slot_state(st, d, slot, tr["p0"] + k, snap), tr["snaps"][k])


ROWS = [(0, 1), (0, 9), (7, 5), (23, 1), (2, 16)]              # (tokens already in the slot, run length)
SLOTS = [3, 0, 6, 2, 5]                                          # slot numbers do not follow the rows


def _all_right(st, d, snap=_snap, same=_same, rows=ROWS, slots=SLOTS, seed=5):
    rng = np.random.default_rng(seed)
    trs = [_trace(st, d, _toks(rng, d, p), _toks(rng, d, 1)[0], c + 1, [s], snap) for (p, c), s in zip(rows, slots)]
    runs = [_right(tr, c) for tr, (_, c) in zip(trs, rows)]
    greedy, nm = st.verify_multi(slots, runs, [tr["p0"] for tr in trs])
    for i, (tr, (_, c)) in enumerate(zip(trs, rows)):
        assert greedy[i] == tr["toks"][1:c + 1], ("greedy", i)
        assert nm[i] == c - 1, ("n_match", i)
    st.commit_multi([c for _, c in rows])
    for tr, (_, c), s in zip(trs, rows, slots):
        _check_slot(st, d, s, tr, c, snap, same)
    ids, lg = st.step_multi(slots, [g[-1] for g in greedy], [tr["p0"] + c for tr, (_, c) in zip(trs, rows)], logits=True)
    for i, (tr, (_, c)) in enumerate(zip(trs, rows)):      # the slots continue as the sequences do
        assert np.array_equal(lg[i].view(U), tr["lg"][c]) and ids[i] == tr["toks"][c + 1], i


@pytest.mark.parametrize("cfg", CFGS + [LA4, DV64])
def test_all_drafts_right(cfg):
    st, eng, orc, keep, d = build(kv_max=64, **cfg)
    st.create_slots(8, 60)
    _all_right(st, d)


def test_partial_acceptance_mixed_in_one_call():
    """the first wrong draft at another index j per row: j < 4 mixes old and kept carried conv inputs; one row keeps nothing"""
    st, eng, orc, keep, d = build(kv_max=64)
    st.create_slots(8, 60)
    rng = np.random.default_rng(7)
    js, slots, pre, c = [1, 2, 3, 5, 7], [4, 1, 7, 0, 3, 6], [3, 0, 11, 6, 20, 2], 9
    trs = [_trace(st, d, _toks(rng, d, p), _toks(rng, d, 1)[0], 13, [s]) for p, s in zip(pre, slots)]
    runs = [_wrong_at(tr, c, j, d["V"]) for tr, j in zip(trs, js)] + [_right(trs[5], c)]
    pos = [tr["p0"] for tr in trs]
    greedy, nm = st.verify_multi(slots, runs, pos)
    for i, j in enumerate(js):
        assert nm[i] == j - 1, (i, nm)
        assert greedy[i][:j] == trs[i]["toks"][1:j + 1], i
    assert nm[5] == c - 1 and greedy[5] == trs[5]["toks"][1:c + 1]
    st.commit_multi(js + [0])
    for tr, j, s in zip(trs, js, slots):
        _check_slot(st, d, s, tr, j)
    _check_slot(st, d, slots[5], trs[5], 0)                   # n_keep = 0: as before the verify
    got = st.generate_multi(slots[:5], [tr["toks"][j] for tr, j in zip(trs, js)], [p + j for p, j in zip(pos, js)], 4)
    for i, (tr, j) in enumerate(zip(trs, js)):
        assert got[i] == tr["toks"][j + 1:j + 5], i
    ids = st.extend_multi([slots[5]], [runs[5]], [pos[5]])      # the dropped row takes the true tokens later
    assert ids[0] == trs[5]["toks"][c]
    _check_slot(st, d, slots[5], trs[5], c)


def test_truncated_commit():
    st, eng, orc, keep, d = build(kv_max=64, seed=2)
    st.create_slots(8, 60)
    rng = np.random.default_rng(9)
    keeps, slots, c = [1, 3, 6], [5, 2, 0], 9
    trs = [_trace(st, d, _toks(rng, d, p), _toks(rng, d, 1)[0], c, [s]) for p, s in zip([4, 0, 9], slots)]
    greedy, nm = st.verify_multi(slots, [_right(tr, c) for tr in trs], [tr["p0"] for tr in trs])
    assert nm == [c - 1] * 3
    st.commit_multi(keeps)                                     # fewer than the verify accepted
    for tr, k, s in zip(trs, keeps, slots):
        _check_slot(st, d, s, tr, k)
    ids, lg = st.step_multi(slots, [tr["toks"][k] for tr, k in zip(trs, keeps)], [tr["p0"] + k for tr, k in zip(trs, keeps)], logits=True)
    for i, (tr, k) in enumerate(zip(trs, keeps)):
        assert np.array_equal(lg[i].view(U), tr["lg"][k]) and ids[i] == tr["toks"][k + 1], i


def test_independence_of_rows_and_the_single_sequence_verify():
    """T = 40 token rows (the router's 32-row form), rows permuted: every row as in a call of that row alone, and as kr_decode_verify on the store's own
    sequence"""
    st, eng, orc, keep, d = build(kv_max=64)
    st.create_slots(8, 60)
    rng = np.random.default_rng(13)
    rows = [(0, 1, None), (0, 9, 4), (7, 5, None), (23, 1, None), (2, 8, 2), (4, 16, 11)]      # (prompt, run length, index of a wrong draft)
    slots, alone_slot = [3, 0, 5, 2, 4, 1], 6
    runs, pos, alone, single = [], [], [], []
    for (p, c, j), s in zip(rows, slots):
        tr = _trace(st, d, _toks(rng, d, p), _toks(rng, d, 1)[0], c, [s, alone_slot])
        run = _right(tr, c) if j is None else _wrong_at(tr, c, j, d["V"])
        g, m = st.verify_multi([alone_slot], [run], [p])
        st.commit_multi([m[0] + 1])
        alone.append((g[0], m[0], _slot_state(st, d, alone_slot, p + m[0] + 1)))
        st.reset_decode_state(d["kv_max"]); st.load_slot(s, p)
        single.append(st.verify(run, p))
        st.commit(1)
        runs.append(run); pos.append(p)
    assert sum(len(r) for r in runs) == 40
    order = [5, 2, 0, 4, 1, 3]
    pick = lambda xs: [xs[i] for i in order]
    greedy, nm = st.verify_multi(pick(slots), pick(runs), pick(pos))
    st.commit_multi([m + 1 for m in nm])
    for r, i in enumerate(order):
        assert greedy[r] == alone[i][0] and nm[r] == alone[i][1], ("alone", i)
        assert (greedy[r], nm[r]) == tuple(single[i]), ("single-sequence verify", i)
        _same(_slot_state(st, d, slots[i], pos[i] + nm[r] + 1), alone[i][2])
    assert [m for _, m, _ in alone] == [0, 3, 4, 0, 1, 10]


@pytest.mark.parametrize("cfg", [dict(), LA4])
def test_cut_invariance_with_the_extend(cfg):
    """verify 9 + commit 4 + extend of the other 5 = one extend of 9"""
    st, eng, orc, keep, d = build(kv_max=64, **cfg)
    st.create_slots(8, 60)
    rng = np.random.default_rng(11)
    tr = _trace(st, d, _toks(rng, d, 6), _toks(rng, d, 1)[0], 9, [0, 1])
    run, p0 = _right(tr, 9), 6
    want = st.extend_multi([1], [run], [p0], logits=True)
    greedy, nm = st.verify_multi([0], [run], [p0])
    assert nm == [8]
    st.commit_multi([4])
    got = st.extend_multi([0], [run[4:]], [p0 + 4], logits=True)
    assert got[0] == want[0] and np.array_equal(got[1].view(U), want[1].view(U))
    _same(_slot_state(st, d, 0, p0 + 9), _slot_state(st, d, 1, p0 + 9))
    _check_slot(st, d, 0, tr, 9)


def test_fp8_kv():
    st, eng, orc, keep, d = build(kv_max=64, seed=3)
    st.set_kv_dtype(True); d["fp8"] = True
    st.create_slots(8, 60)
    _all_right(st, d)


def test_mla():
    st, eng, keep, d = mla._build(False, kv_max=64, **mla.CFGS[1])
    st.create_slots(8, 60)
    _all_right(st, d, snap=mla._snap, same=mla._same)


def test_multi_attn_fast_option():
    """slots of max_seq > gqa_split_min under the option: every token carries the bits extend_multi gives it under the option"""
    st, eng, orc, keep, d = build(kv_max=64, seed=6)
    st.create_slots(4, 1030)
    rng = np.random.default_rng(17)
    tr = _trace(st, d, _toks(rng, d, 5), _toks(rng, d, 1)[0], 9, [0, 1, 2])
    p0 = 5
    st.set_option("multi_attn_fast", 1)
    try:
        run, ids = [tr["toks"][0]], []
        for k in range(9):                                     # the yardstick: the option's own greedy stream, token by token
            ids.append(st.extend_multi([2], [[run[k]]], [p0 + k])[0])
            run.append(ids[-1])
        run = run[:9]
        greedy, nm = st.verify_multi([0], [run], [p0])
        assert greedy[0] == ids and nm == [8]
        st.commit_multi([6])
        st.extend_multi([1], [run[:6]], [p0])
        _same(_slot_state(st, d, 0, p0 + 6), _slot_state(st, d, 1, p0 + 6))
        a = st.step_multi([0], [run[6]], [p0 + 6], logits=True)
        b = st.step_multi([1], [run[6]], [p0 + 6], logits=True)
        assert a[0] == b[0] == [ids[6]] and np.array_equal(a[1].view(U), b[1].view(U))
    finally:
        st.set_option("multi_attn_fast", 0)


def _fill(st, d, prompts, slot_lists):
    for p, slots in zip(prompts, slot_lists):
        st.reset_decode_state(d["kv_max"])
        if p:
            st.prefill(p, 0)
        for s in slots:
            st.save_slot(s, len(p))


@pytest.mark.parametrize("max_draft", [1, 4, 15])
def test_generate_multi_lookup_equals_generate_multi(max_draft):
    st, eng, orc, keep, d = build(kv_max=64, seed=1)
    st.create_slots(8, 60)
    rng = np.random.default_rng(23)
    n_tok = 12
    prompts = [_toks(rng, d, p) for p in (5, 0, 9, 60 - n_tok)]      # the last row ends at the slot boundary
    firsts, pos = _toks(rng, d, 4), [len(p) for p in prompts]
    A, B = [6, 1, 4, 3], [0, 7, 2, 5]
    for repeat, stop in ((True, False), (False, False), (True, True)):
        _fill(st, d, prompts, [[a, b] for a, b in zip(A, B)])
        want = st.generate_multi(B, firsts, pos, n_tok)
        stops = ()
        if stop:      # a stop id that row 0 first emits at index k >= 2: inside the draft its first pass accepts (max_draft 1: in a later pass)
            k = next(k for k in range(2, n_tok) if want[0].index(want[0][k]) == k)
            stops = (want[0][k],)
            _fill(st, d, prompts, [[b] for b in B])
            want = st.generate_multi(B, firsts, pos, n_tok, stop_ids=stops)
            assert len(want[0]) == k + 1
        # contexts that hold the row's greedy stream (every draft right), or contexts that do not
        ctx = [[f] + w for f, w in zip(firsts, want)] if repeat else [_toks(rng, d, 20) for _ in range(4)]
        got = st.generate_multi_lookup(A, firsts, pos, n_tok, contexts=ctx, max_draft=max_draft, stop_ids=stops)
        assert got == want
        for a, b, p, w in zip(A, B, pos, want):
            _same(_slot_state(st, d, a, p + len(w)), _slot_state(st, d, b, p + len(w)))
        stats = st.last_multi_lookup_stats
        if repeat:                                             # it did speculate
            assert stats["passes"] < n_tok and all(a > 0 for a in stats["accepted"]), stats


def test_generate_multi_lookup_without_contexts():
    st, eng, orc, keep, d = build(kv_max=64, seed=1)
    st.create_slots(4, 60)
    rng = np.random.default_rng(29)
    prompts, firsts = [_toks(rng, d, 3), _toks(rng, d, 8)], _toks(rng, d, 2)
    _fill(st, d, prompts, [[0, 1], [2, 3]])
    want = st.generate_multi([1, 3], firsts, [3, 8], 20)
    assert st.generate_multi_lookup([0, 2], firsts, [3, 8], 20) == want
    for a, b, p in ((0, 1, 3), (2, 3, 8)):
        _same(_slot_state(st, d, a, p + 20), _slot_state(st, d, b, p + 20))


def test_refusals_and_the_pending_state():
    st, eng, orc, keep, d = build(kv_max=32)
    with pytest.raises(RuntimeError, match="no sequence slots"):
        st.verify_multi([0], [[1, 2]], [0])
    st.create_slots(3, 24)
    with pytest.raises(RuntimeError, match="no verify over slots is pending"):
        st.commit_multi([1])
    st.fill_state_synthetic(d["kv_max"], seed=5)
    st.save_slot(1, 20)
    st.fill_state_synthetic(d["kv_max"], seed=6)
    st.save_slot(2, 10)
    state = lambda: (_slot_state(st, d, 1, 20), _slot_state(st, d, 2, 10))
    want = state()

    def unchanged():
        for g, w in zip(state(), want):
            _same(g, w)

    V = d["V"]
    refused = [
        (([1, 2], [[3], []], [20, 10]), "row 1"),                                           # a count of 0
        (([1], [[3] * (KR_VERIFY_MAX + 1)], [2]), "row 0"),                                 # a count of 17
        (([1] * 65, [[1] * 16] * 65, [0] * 65), "row 64"),                                  # T = 1040 > KR_EXTEND_MAX_TOKENS
        (([1, 1], [[3], [4]], [20, 21]), "row 1"),                                          # a slot named twice
        (([2, 1], [[3], [1, 2, 3, 4, 5]], [10, 20]), "row 1"),                              # last position == max_seq
        (([1], [[2, V, 3]], [20]), "row 0"),                                                # a draft token outside the vocabulary
    ]
    for args, row in refused:
        with pytest.raises(ValueError, match=row):
            st.verify_multi(*args)
        unchanged()                                            # (load_slot inside: nothing is pending either)
    st.set_attention_mode(fast=True)                           # a tolerance bit
    try:
        with pytest.raises(RuntimeError, match="exact-mode only"):
            st.verify_multi([1], [[2, 3]], [20])
    finally:
        st.set_attention_mode(False)
    unchanged()
    greedy, nm = st.verify_multi([1, 2], [[2, 3, 4], [5, 6]], [20, 10])
    pending = [
        lambda: st.step_multi([1], [2], [20]),
        lambda: st.step_multi_sample([1], [2], [20]),
        lambda: st.extend_multi([1], [[2, 3]], [20]),
        lambda: st.generate_multi([1], [2], [20], 2),
        lambda: st.generate_multi([1], [2], [20], 2, temperature=0.7, rng_seeds=5),
        lambda: st.generate_multi_lookup([1], [2], [20], 2),
        lambda: st.save_slot(0, 4),
        lambda: st.load_slot(1, 20),
        lambda: st.set_slot_sampler(1, 2, 0.8, 20, 0.9, 0.5, 7),
        lambda: st.verify_multi([0], [[1]], [0]),
    ]
    for call in pending:
        with pytest.raises(RuntimeError, match="verify over slots is pending"):
            call()
    with pytest.raises(ValueError, match="row 0"):             # out of range: names its row, applies nothing, stays pending
        st.commit_multi([nm[0] + 2, 0])
    with pytest.raises(ValueError, match="row 1"):
        st.commit_multi([0, -1])
    with pytest.raises(RuntimeError, match="verify over slots is pending"):
        st.step_multi([1], [2], [20])
    st.commit_multi([0, 0])
    unchanged()                                                # every refused call and the dropped verify left the slots as they were
    with pytest.raises(RuntimeError, match="no verify over slots is pending"):
        st.commit_multi([0, 0])
    st.verify_multi([1], [[2, 3]], [20])
    st.create_slots(3, 24)                                     # drops the pending verify with the slots
    assert len(st.step_multi([1], [2], [0])) == 1


def test_the_store_sequence_is_untouched_and_steps_while_pending():
    st, eng, orc, keep, d = build(kv_max=48)
    st.create_slots(2, 40)
    rng = np.random.default_rng(31)
    tr = _trace(st, d, _toks(rng, d, 7), _toks(rng, d, 1)[0], 6, [1])
    own = _toks(rng, d, 6)
    st.reset_decode_state(d["kv_max"])
    st.prefill(own, 0)                                         # the store's own sequence: something else
    own_state = lambda: (st.read_logits().view(U).copy(), st.last_token(), _snap(st, d, 48))
    before = own_state()
    st.decode_step(before[1], 6)
    stepped = own_state()
    st.reset_decode_state(d["kv_max"])
    st.prefill(own, 0)
    greedy, nm = st.verify_multi([1], [_right(tr, 6)], [7])
    after = own_state()
    assert np.array_equal(before[0], after[0]) and before[1] == after[1]
    _same(after[2], before[2])
    st.decode_step(after[1], 6)                                # the store's own entry points run while the slots wait for their commit
    st.commit_multi([5])
    after = own_state()
    assert np.array_equal(stepped[0], after[0]) and stepped[1] == after[1]
    _same(after[2], stepped[2])
    _check_slot(st, d, 1, tr, 5)
