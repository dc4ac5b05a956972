"""The "multi_attn_exact_split" option (docs/design/30-multi-attn-exact-split.md): wherever a batched pass over device slots would launch the exact per-slot GQA
attention kernel it launches three -- scores spread over position tiles, the softmax one wave per (row, head), P.V spread over heads and head-dim slices.  No bit
changes: every call gives what the same call gives with the option off -- ids, logits, every K / V row, every conv and recurrent state -- in steps, extends, verify
passes and generation, on flat, paged and forked slots, FP16 and E4M3 caches.  There is no tolerance in this file.

The reference is never the new path: it is the same call with the option off on equally filled slots and, in test 1, also the store's own decode_step on each
sequence alone (computed once per geometry and shared).  Every comparison is on ids and u32 / stored-row bit patterns.  Every test sets
"multi_attn_exact_split_min" to 1, so these small caches take the split."""
import functools

import numpy as np
import pytest

from tests.test_decode_gpu import build
from tests.test_multi_paged_gpu import _state_error
from tests.test_speculative_gpu import _same, _snap

pytestmark = pytest.mark.gpu
U = np.uint32
OPT, MIN = "multi_attn_exact_split", "multi_attn_exact_split_min"
# the kernels' tile constants (kr_multi_split.hip, kr_multi_softmax_dev.h): positions per scores workgroup, per P.V stage, the padding of a score row, the softmax tile
SCORE_TILE, PV_STAGE, ROW_PAD, SOFTMAX_TILE = 256, 64, 32, 1024
KV_MAX = 600                                                                # two full score tiles and 88 positions
LONG_KV = 1100                                                              # above the softmax tile, and above gqa_split_min
# (head_dim, query heads on 2 KV heads, E4M3): G = 8, 4, 2, 1, 32, all three head dims, both cache types
MODELS = [(256, 16, False), (128, 8, True), (64, 4, False), (64, 2, True), (64, 64, False)]


def _around(edge):
    """the positions whose row attends over edge - 1, edge and edge + 1 positions"""
    return [edge - 2, edge - 1, edge]


# one position below, at and above: the 32-position padding of a score row, the P.V stage, the first and the second scores tile; position 0; the slot's last
POS = sorted({0, KV_MAX - 1, *_around(ROW_PAD), *_around(PV_STAGE), *_around(SCORE_TILE), *_around(2 * SCORE_TILE)})
POS_LONG = sorted({0, LONG_KV - 1, *_around(SOFTMAX_TILE), *_around(3 * SCORE_TILE)})      # the softmax tile's edge, one geometry
SLOTS = [5, 12, 0, 7, 2, 14, 9, 3, 11, 6, 1, 13, 4, 10, 8, 15]              # slot numbers do not follow the rows
assert len(POS) <= len(SLOTS) and len(POS_LONG) <= len(SLOTS)

_stores = []
ALL_OPTS = (OPT, "multi_extend_exact_mfma", "multi_extend_flash", "multi_attn_fast", "multi_attn_fast_paged")


@pytest.fixture(autouse=True)
def options_off_afterwards():
    yield
    for st in _stores:
        for o in ALL_OPTS:
            st.set_option(o, 0)
        st.set_option(MIN, 1)
        st.set_attention_mode(False)


def _bits(x):
    return np.ascontiguousarray(x).view(U).copy()


def _pages(n, pt):
    return (n + pt - 1) // pt


@functools.lru_cache(maxsize=None)
def _model(hd, nh, fp8, kv_max=KV_MAX, kinds=("gqa", "gqa")):
    """one store per geometry, built once and shared"""
    st, eng, orc, keep, d = build(seed=3, hd=hd, nh=nh, kv_max=kv_max, kinds=list(kinds))
    if fp8:
        st.set_kv_dtype(True); d["fp8"] = True
    st.set_option(MIN, 1)
    _stores.append(st)
    return st, (eng, orc, keep), d


@functools.lru_cache(maxsize=None)
def _seq(hd, nh, fp8, kv_max=KV_MAX):
    """the one token sequence of a geometry: row p of every test consumes token p behind the prefix [0, p)"""
    d = _model(hd, nh, fp8, kv_max)[2]
    return tuple(int(x) for x in np.random.default_rng(hd + nh + kv_max).integers(0, d["V"], kv_max))


@functools.lru_cache(maxsize=None)
def _single(hd, nh, fp8, kv_max=KV_MAX):
    """the single-sequence reference, computed once and never modified: the sequence by the store's own exact prompt pass, the token at every position of POS by
    decode_step -> {position: (logits bits, greedy id)}, and the K / V rows of the whole sequence"""
    st, _, d = _model(hd, nh, fp8, kv_max)
    seq, at, out = list(_seq(hd, nh, fp8, kv_max)), 0, {}
    st.reset_decode_state(kv_max)
    for p in (POS if kv_max == KV_MAX else POS_LONG):
        if p > at:
            st.prefill(seq[at:p], at)
        st.decode_step(seq[p], p)
        out[p] = (_bits(st.read_logits()), st.last_token())
        at = p + 1
    return out, _snap(st, d, kv_max)


def _fill(st, d, seq, want):
    """want = [(slot, n)]: the first n tokens of seq, by the exact prompt pass on the store's own sequence, into the slot (GQA stores: one pass serves every n)"""
    st.reset_decode_state(d["kv_max"])
    top = max(n for _, n in want)
    if top:
        st.prefill(list(seq[:top]), 0)
    for s, n in want:
        st.save_slot(s, n)


def _slot_state(st, d, slot, upto):
    st.reset_decode_state(d["kv_max"])
    st.load_slot(slot, upto)
    return _snap(st, d, upto)


def _upto(snap, n):
    return [(k, li, a[:n], b[:n]) for k, li, a, b in snap]


def _equal(a, b, where=""):
    """two results (ids, logits, slot states) of one scenario: bit for bit"""
    assert [int(x) for x in a[0]] == [int(x) for x in b[0]], ("ids", where)
    assert np.array_equal(_bits(a[1]), _bits(b[1])), ("logits", where)
    assert len(a[2]) == len(b[2])
    for x, y in zip(a[2], b[2]):
        _same(x, y)


def _off_on(st, scenario, **other):
    """scenario(st) -> (ids, logits, states) on slots it creates and fills itself, once with the option off and once with it on; `other` options stay set for both"""
    out = []
    for on in (0, 1):
        for o, v in other.items():
            st.set_option(o, v)
        st.set_option(OPT, on)
        out.append(scenario(st))
        st.set_option(OPT, 0)
        for o in other:
            st.set_option(o, 0)
    return out


def _steps(st, d, seq, pos, n_slots=16, kv_max=KV_MAX, **slots_kw):
    """one step_multi: row i consumes token pos[i] of seq at position pos[i] in slot SLOTS[i] -> (ids, logits, states)"""
    st.create_slots(n_slots, kv_max, **slots_kw)
    slots = SLOTS[:len(pos)]
    _fill(st, d, seq, list(zip(slots, pos)))
    ids, lg = st.step_multi(slots, [seq[p] for p in pos], list(pos), logits=True)
    return ids, lg, [_slot_state(st, d, s, p + 1) for s, p in zip(slots, pos)]


# ---- 1: on == off == decode_step on each sequence alone ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hd,nh,fp8,kv_max", [m + (KV_MAX,) for m in MODELS] + [(128, 8, True, LONG_KV)])
def test_step_multi_equals_option_off_and_decode_step(hd, nh, fp8, kv_max):
    """rows at every edge position in one call, slots scrambled: logits and ids bit for bit, then every K / V row of every slot"""
    st, _, d = _model(hd, nh, fp8, kv_max)
    seq, (single, snap) = _seq(hd, nh, fp8, kv_max), _single(hd, nh, fp8, kv_max)
    pos = POS if kv_max == KV_MAX else POS_LONG
    took = []      # not vacuous: the pass took the option's form in the on-leg and not in the off-leg (multi_path_counts)

    def counted(st):
        st.multi_path_counts(reset=True)
        out = _steps(st, d, seq, pos, kv_max=kv_max)
        took.append(st.multi_path_counts()["xs_split"])
        return out

    off, on = _off_on(st, counted)
    assert took == [0, 1], ("xs_split", took)
    _equal(on, off)
    for i, p in enumerate(pos):
        assert np.array_equal(_bits(on[1][i]), single[p][0]) and int(on[0][i]) == single[p][1], ("decode_step", p)
        _same(on[2][i], _upto(snap, p + 1))


# ---- 2: mixed passes through extend_multi -------------------------------------------------------------------------------------------------------------------
# (position of the first token, tokens): unit rows at the edges, runs across the scores-tile, P.V-stage and padding edges
MIXED = [(255, 1), (250, 10), (0, 1), (60, 70), (256, 1), (0, 2), (63, 1), (31, 1), (500, 30)]
RUNS_ONLY = [(254, 3), (30, 40), (510, 5)]
UNITS_ONLY = [(511, 1), (64, 1), (0, 1), (257, 1)]


@pytest.mark.parametrize("other", [None, "multi_extend_exact_mfma", "multi_extend_flash"])
@pytest.mark.parametrize("hd,nh,fp8", MODELS)
def test_mixed_passes_through_extend_multi(hd, nh, fp8, other):
    """unit rows beside runs with no run option, with "multi_extend_exact_mfma" and with "multi_extend_flash": on == off with the same other option; a pass with
    no unit row and a pass of unit rows only among them"""
    st, _, d = _model(hd, nh, fp8)
    seq = _seq(hd, nh, fp8)

    def scenario(st):
        st.create_slots(16, KV_MAX)
        ids, lgs, states, at = [], [], [], 0
        for rows in (MIXED, RUNS_ONLY, UNITS_ONLY):
            slots = SLOTS[at:at + len(rows)]
            at += len(rows)
            _fill(st, d, seq, [(s, p) for s, (p, _) in zip(slots, rows)])
            i, lg = st.extend_multi(slots, [list(seq[p:p + c]) for p, c in rows], [p for p, _ in rows], logits=True)
            ids += list(i); lgs.append(lg)
            states += [_slot_state(st, d, s, p + c) for s, (p, c) in zip(slots, rows)]
        return ids, np.concatenate(lgs), states

    off, on = _off_on(st, scenario, **({other: 1} if other else {}))
    _equal(on, off, other)


# ---- 3: verify ----------------------------------------------------------------------------------------------------------------------------------------------
VERIFY_POS = [254, 255, 510, 62, 0]                                         # runs of 3: two rows of one run attend over different lengths of the slot, across a tile edge


@pytest.mark.parametrize("sample", [False, True])
@pytest.mark.parametrize("hd,nh,fp8", [MODELS[0], MODELS[1], MODELS[4]])
def test_verify_and_commit(hd, nh, fp8, sample):
    """verify_multi + commit_multi / verify_multi_sample: a verify with drafts from the sequence, committed as nothing; then one whose drafts are the ids the first
    returned (every draft matches), committed at different lengths: ids, n_match and the states after the commit on == off"""
    st, _, d = _model(hd, nh, fp8)
    seq = _seq(hd, nh, fp8)

    def scenario(st):
        st.create_slots(16, KV_MAX)
        slots = SLOTS[:len(VERIFY_POS)]
        _fill(st, d, seq, list(zip(slots, VERIFY_POS)))
        if sample:
            for i, s in enumerate(slots):
                st.set_slot_sampler(s, seq[VERIFY_POS[i]], 0.8, 40, 0.95, 0.5, 100 + i)
        verify = st.verify_multi_sample if sample else st.verify_multi
        g1, nm1 = verify(slots, [list(seq[p:p + 3]) for p in VERIFY_POS], VERIFY_POS)
        st.commit_multi([0] * len(slots))
        ids = [x for row, m in zip(g1, nm1) for x in row[:m + 1]] + list(nm1)
        keep = [1] * len(slots)
        if not sample:      # the greedy continuation, one token further per pass: the last pass's drafts all match
            g2, _ = verify(slots, [[seq[p], row[0], seq[p + 2]] for p, row in zip(VERIFY_POS, g1)], VERIFY_POS)
            st.commit_multi([0] * len(slots))
            g3, nm3 = verify(slots, [[seq[p], row[0], row[1]] for p, row in zip(VERIFY_POS, g2)], VERIFY_POS)
            assert list(nm3) == [2] * len(slots)
            keep = [3, 2, 1, 3, 2]
            ids += [x for row in list(g2) + list(g3) for x in row] + list(nm3)
        else:
            g2, nm2 = verify(slots, [list(seq[p:p + 3]) for p in VERIFY_POS], VERIFY_POS)
            ids += [x for row, m in zip(g2, nm2) for x in row[:m + 1]] + list(nm2)
        st.commit_multi(keep)
        return ids, np.zeros(1, np.float32), [_slot_state(st, d, s, p + k) for s, p, k in zip(slots, VERIFY_POS, keep)]

    off, on = _off_on(st, scenario)
    _equal(on, off, "verify + commit")


# ---- 4: generation ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lookup", [False, True])
@pytest.mark.parametrize("hd,nh,fp8", [MODELS[1], MODELS[2]])
def test_generate_multi_across_a_tile_edge(hd, nh, fp8, lookup):
    """8 tokens from positions 252 (across the scores tile's edge), 60 (the P.V stage's), 508 and 0, by generate_multi and by the lookup loop (steps and verify
    passes): tokens and end states on == off"""
    st, _, d = _model(hd, nh, fp8)
    seq = _seq(hd, nh, fp8)
    starts = [252, 60, 508, 0]

    def scenario(st):
        st.create_slots(16, KV_MAX)
        slots = SLOTS[:len(starts)]
        _fill(st, d, seq, list(zip(slots, starts)))
        firsts = [seq[p] for p in starts]
        if lookup:
            toks = st.generate_multi_lookup(slots, firsts, starts, 8, contexts=[list(seq[:p + 1]) for p in starts])
        else:
            toks = st.generate_multi(slots, firsts, starts, 8)
        return [x for row in toks for x in row], np.zeros(1, np.float32), [_slot_state(st, d, s, p + 8) for s, p in zip(slots, starts)]

    off, on = _off_on(st, scenario)
    _equal(on, off, "generate")


# ---- 5: paged slots -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("page_tokens", [32, 64, 256])
@pytest.mark.parametrize("hd,nh,fp8", MODELS)
def test_paged_and_forked_slots(hd, nh, fp8, page_tokens):
    """page_tokens 32: a P.V stage spans two pages and a scores tile eight; 64: a stage is a page; 256: a scores tile is a page.  Scrambled placement: a spare
    slot saved before the 512-token prefix and trimmed after it leaves a hole, and a page saved right behind the prefix stays held, so the page the step at
    position 512 maps does not follow the slot's others.  Then a fork at position 300 (no page edge) with the step on the dst: dst on == off, and the src's rows
    are unchanged"""
    st, _, d = _model(hd, nh, fp8)
    seq, (single, snap) = _seq(hd, nh, fp8), _single(hd, nh, fp8)
    pt, far, fork_at = page_tokens, 2 * SCORE_TILE, 300
    others = [p for p in POS if p != far]

    def scenario(st):
        spare, dst = SLOTS[len(POS)], SLOTS[len(POS) + 1]
        need = sum(_pages(p + 1, pt) for p in POS) + _pages(100, pt) + 1 + _pages(fork_at + 1, pt)
        st.create_slots(16, KV_MAX, page_tokens=pt, n_pages=need + 2)
        st.reset_decode_state(d["kv_max"])
        st.prefill(list(seq[:KV_MAX - 1]), 0)
        slot_of = dict(zip(POS, SLOTS))
        for p in others:
            st.save_slot(slot_of[p], p)
        st.save_slot(spare, min(100, pt))
        st.save_slot(slot_of[far], far)
        st.save_slot(dst, 1)
        st.trim_slot(spare, 0)
        ids, lg = st.step_multi([slot_of[p] for p in POS], [seq[p] for p in POS], list(POS), logits=True)
        used = [int(x) for x in st.slot_page_ids(slot_of[far])[0][:_pages(far + 1, pt)]]
        assert min(used) >= 0 and used != list(range(used[0], used[0] + len(used))), ("the long slot's pages are consecutive", used)
        states = [_slot_state(st, d, slot_of[p], p + 1) for p in POS]
        for p in others:
            st.trim_slot(slot_of[p], 0)
        st.trim_slot(dst, 0)
        st.fork_slot(slot_of[far], [dst], fork_at)
        ids2, lg2 = st.step_multi([dst], [seq[fork_at]], [fork_at], logits=True)
        states += [_slot_state(st, d, dst, fork_at + 1), _slot_state(st, d, slot_of[far], far + 1)]
        return list(ids) + list(ids2), np.concatenate([lg, lg2]), states

    off, on = _off_on(st, scenario)
    _equal(on, off, ("paged", pt))
    for i, p in enumerate(POS):
        assert np.array_equal(_bits(on[1][i]), single[p][0]), ("decode_step", p)
    _same(on[2][-1], _upto(snap, far + 1))              # the fork's src: untouched
    _same(on[2][-2], _upto(snap, fork_at + 1))          # the dst: the same sequence, one row behind the fork point


# ---- 6: a hybrid store --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fp8", [False, True])
def test_hybrid_store(fp8):
    """linear attention + GQA: two steps in a row, on == off including conv and recurrent state"""
    st, _, d = _model(64, 4, fp8, kinds=("la", "gqa", "la", "gqa"))
    seq = _seq(64, 4, fp8)
    pos, slots = [0, 31, 64, 255, 256, 300], [3, 0, 5, 1, 4, 2]

    def scenario(st):
        st.create_slots(6, KV_MAX)
        for s, p in zip(slots, pos):
            _fill(st, d, seq, [(s, p)])      # the recurrent state belongs to its prefix: one pass each
        ids, lg = st.step_multi(slots, [seq[p] for p in pos], pos, logits=True)
        ids2, lg2 = st.step_multi(slots, list(ids), [p + 1 for p in pos], logits=True)
        return list(ids) + list(ids2), np.concatenate([lg, lg2]), [_slot_state(st, d, s, p + 2) for s, p in zip(slots, pos)]

    off, on = _off_on(st, scenario)
    _equal(on, off, "hybrid")


# ---- 7: stale scratch ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hd,nh,fp8", MODELS)
def test_short_call_after_a_long_one(hd, nh, fp8):
    """a call at positions 599 and 512 leaves scores and probabilities in the scratch; the call at positions 5, 40 and 31 after it uses another row stride over
    the same bytes and is on == off: nothing beyond a row's own positions is consumed"""
    st, _, d = _model(hd, nh, fp8)
    seq = _seq(hd, nh, fp8)

    def scenario(st):
        st.create_slots(16, KV_MAX)
        long_pos, short_pos = [KV_MAX - 1, 2 * SCORE_TILE], [5, 40, 31]
        _fill(st, d, seq, list(zip([2, 4, 1, 6, 3], long_pos + short_pos)))
        st.step_multi([2, 4], [seq[p] for p in long_pos], long_pos)
        ids, lg = st.step_multi([1, 6, 3], [seq[p] for p in short_pos], short_pos, logits=True)
        return ids, lg, [_slot_state(st, d, s, p + 1) for s, p in zip([1, 6, 3], short_pos)]

    off, on = _off_on(st, scenario)
    _equal(on, off, "short after long")


# ---- 8: the threshold ---------------------------------------------------------------------------------------------------------------------------------------
def test_threshold_above_and_below_the_call():
    """with "multi_attn_exact_split_min" above every position of the call the pass keeps the one kernel; at 1 it takes the split: both equal the option-off call"""
    hd, nh, fp8 = MODELS[1]
    st, _, d = _model(hd, nh, fp8)
    seq = _seq(hd, nh, fp8)
    pos = [0, 255, 256, 300]
    off = _steps(st, d, seq, pos)
    st.set_option(OPT, 1)
    st.set_option(MIN, KV_MAX + 1)
    above = _steps(st, d, seq, pos)
    st.set_option(MIN, 301)                                                 # exactly the call's longest attention
    at = _steps(st, d, seq, pos)
    st.set_option(MIN, 1)
    one = _steps(st, d, seq, pos)
    st.set_option(OPT, 0)
    _equal(above, off, "above")
    _equal(at, off, "at")
    _equal(one, off, "1")


def test_minimum_below_one_is_a_value_error():
    st, _, d = _model(64, 4, False, kv_max=32)
    for v in (0, -5):
        with pytest.raises(ValueError) as e:
            st.set_option(MIN, v)
        assert MIN in str(e.value), str(e.value)


# ---- 9: refusals --------------------------------------------------------------------------------------------------------------------------------------------
def _calls(st, V):
    t = lambda k: [x % V for x in range(1, 1 + k)]
    return (lambda: st.step_multi([1], t(1), [0]), lambda: st.extend_multi([1], [t(3)], [0]), lambda: st.generate_multi([1], t(1), [0], 2),
            lambda: st.verify_multi([1], [t(2)], [0]), lambda: st.generate_multi_lookup([1], t(1), [0], 2))


def _refused_then_fine(st, d, arm, refuse, clear):
    """a slot holding a prefix (filled with nothing set); after arm() every batched call is refused by refuse(call); after clear() the slot's state is what it was
    and the run succeeds"""
    st.create_slots(2, 20)
    _fill(st, d, [3, 1, 4], [(1, 3)])
    before = _slot_state(st, d, 1, 3)
    arm()
    for call in _calls(st, d["V"]):
        refuse(call)
    clear()
    _same(_slot_state(st, d, 1, 3), before)
    st.extend_multi([1], [[1, 2, 3]], [3])


def test_store_without_gqa_layers_is_refused():
    st, _, d = _model(64, 4, False, kv_max=32, kinds=("la", "la"))
    _refused_then_fine(st, d, lambda: st.set_option(OPT, 1), lambda call: _state_error(call, OPT, "has none"), lambda: st.set_option(OPT, 0))


def test_mode_bits_stay_refused_with_their_old_text():
    st, _, d = _model(64, 4, False, kv_max=32)

    def arm():
        st.set_option(OPT, 1); st.set_attention_mode(True)

    _refused_then_fine(st, d, arm, lambda call: _state_error(call, "exact-mode only"), lambda: st.set_attention_mode(False))      # the option itself stays set
    st.set_option(OPT, 0)


# ---- 10: long slots, the flash-decode claims the unit rows --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("paged", [False, True])
def test_long_slots_under_multi_attn_fast(paged):
    """slots of 1100 positions (above gqa_split_min) with "multi_attn_fast" (flat) / "multi_attn_fast_paged" (pages of 64) also set: the rows take the split-KV
    flash-decode, the split has nothing to do, nothing is refused, and the call equals the one under that option alone -- which differs from the exact call"""
    hd, nh, fp8 = 128, 8, True
    st, _, d = _model(hd, nh, fp8, LONG_KV)
    seq = _seq(hd, nh, fp8, LONG_KV)
    pos = [1030, 40, SOFTMAX_TILE, 700]
    kw = dict(page_tokens=64, n_pages=sum(_pages(p + 1, 64) for p in pos) + 2) if paged else {}
    fast = "multi_attn_fast_paged" if paged else "multi_attn_fast"
    scenario = lambda st: _steps(st, d, seq, pos, n_slots=16, kv_max=LONG_KV, **kw)
    exact = scenario(st)
    fd, both = _off_on(st, scenario, **{fast: 1})
    _equal(both, fd, fast)
    assert any(not np.array_equal(_bits(fd[1][r]), _bits(exact[1][r])) for r in range(len(pos)))      # the flash-decode did run
