"""The "multi_mla_exact_split" option (docs/design/31-multi-mla-exact-split.md): wherever a batched pass over device slots would launch the exact per-slot MLA
attention kernel it launches three -- scores spread over position tiles and head groups, the softmax one wave per (row, head), the weighted sum spread over
heads and latent slices.  No bit changes: every call gives what the same call gives with the option off -- ids, logits, every latent and rope-key row, sampler
state -- in steps, extends, verify passes and generation, on flat, paged and forked slots, FP16 and E4M3 caches, kv_lora_rank 512 / 256, the direct and the LoRA
query path, a ragged last head group included.  There is no tolerance in this file.

The reference is never the new path: it is the same call with the option off on equally filled slots and, in test 1, also the store's own decode_step on each
sequence alone (computed once per geometry and shared).  Every comparison is on ids and u32 / stored-row bit patterns.  Every test sets
"multi_mla_exact_split_min" to 1, so these small caches take the split."""
import functools

import numpy as np
import pytest

import tests.test_multi_mla_gpu as MM
from tests.test_multi_paged_gpu import Mla, _slot_state, _state_error

pytestmark = pytest.mark.gpu
U = np.uint32
OPT, MIN = "multi_mla_exact_split", "multi_mla_exact_split_min"
# the kernels' tile constants (kr_multi_mla_split.hip, kr_multi_softmax_dev.h): the padding of a score row = the rows of a scores stage, positions per scores
# workgroup = per stage of the weighted sum, the softmax tile; the weighted sum takes 32 heads a pass
ROW_PAD, SCORE_STAGE, SCORE_TILE, PV_STAGE, SOFTMAX_TILE, PV_HEADS = 32, 32, 64, 64, 1024, 32
KV_MAX = 600                                                                # nine full score tiles and 24 positions
LONG_KV = 1100                                                              # above the softmax tile, and above mla_split_min
FAR = 8 * SCORE_TILE                                                        # a page edge of every page size of test 5
# (kv_lora_rank, heads, LoRA query path, E4M3): one to four heads of a group, 11 = a ragged last head group, 40 = a second pass of the weighted sum (above 32
# heads) with 8 heads in it
MODELS = [(512, 4, False, False), (256, 2, False, True), (512, 16, True, True), (256, 1, False, False), (512, 11, False, True), (256, 40, False, True)]
LONG_MODEL = (512, 4, False, True)
assert MODELS[-1][1] > PV_HEADS


def _around(edge):
    """the positions whose row attends over edge - 1, edge and edge + 1 positions"""
    return [edge - 2, edge - 1, edge]


# one position below, at and above: the 32-position padding of a score row (= the scores stage), the scores tile (= the stage of the weighted sum), the second
# scores tile; position 0; the ninth tile's first position; the slot's last
POS = sorted({0, KV_MAX - 1, FAR, *_around(ROW_PAD), *_around(SCORE_TILE), *_around(2 * SCORE_TILE)})
POS_LONG = sorted({0, LONG_KV - 1, *_around(SOFTMAX_TILE), *_around(3 * SCORE_TILE)})      # the softmax tile's edge, one geometry
SLOTS = [5, 12, 0, 7, 2, 14, 9, 3, 11, 6, 1, 13, 4, 10, 8, 15]              # slot numbers do not follow the rows
assert len(POS) + 2 <= len(SLOTS) and len(POS_LONG) <= len(SLOTS)

_stores = []
ALL_OPTS = (OPT, "multi_extend_mla_exact_mfma", "multi_extend_mla_flash", "multi_mla_fast")


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


def _model(klr, nh, lora, fp8, kv_max=KV_MAX):
    return _model_c(klr, nh, lora, fp8, kv_max)      # one cache entry however the call spells kv_max


@functools.lru_cache(maxsize=None)
def _model_c(klr, nh, lora, fp8, kv_max):
    """one store per geometry, built once and shared"""
    st, eng, keep, d = MM._build(fp8, seed=3, klr=klr, nh=nh, lora=lora, kv_max=kv_max)
    st.set_option(MIN, 1)
    _stores.append(st)
    return st, (eng, keep), d


def _seq(klr, nh, lora, fp8, kv_max=KV_MAX):
    return _seq_c(klr, nh, lora, fp8, kv_max)      # one cache entry however the call spells kv_max


@functools.lru_cache(maxsize=None)
def _seq_c(klr, nh, lora, fp8, kv_max):
    """the one token sequence of a geometry: row p of every test consumes token p behind the prefix [0, p)"""
    d = _model(klr, nh, lora, fp8, kv_max)[2]
    return tuple(int(x) for x in np.random.default_rng(klr + nh + kv_max).integers(0, d["V"], kv_max))


def _single(klr, nh, lora, fp8, kv_max=KV_MAX):
    return _single_c(klr, nh, lora, fp8, kv_max)      # one cache entry however the call spells kv_max


@functools.lru_cache(maxsize=None)
def _single_c(klr, nh, lora, fp8, kv_max):
    """the single-sequence reference, computed once and never modified: the sequence by the store's own exact prompt pass, the token at every position of POS by
    decode_step -> {position: (logits bits, greedy id)}, and the latent / rope-key rows of the whole sequence"""
    st, _, d = _model(klr, nh, lora, fp8, kv_max)
    seq, at, out = list(_seq(klr, nh, lora, fp8, kv_max)), 0, {}
    st.reset_decode_state(kv_max)
    for p in (POS if kv_max == KV_MAX else POS_LONG):
        if p > at:
            st.prefill(seq[at:p], at)
        st.decode_step(seq[p], p)
        out[p] = (_bits(st.read_logits()), st.last_token())
        at = p + 1
    return out, MM._snap(st, d, kv_max)


def _fill(st, d, seq, want):
    """want = [(slot, n)]: the first n tokens of seq, by the exact prompt pass on the store's own sequence, into the slot (one pass serves every n)"""
    st.reset_decode_state(d["kv_max"])
    top = max(n for _, n in want)
    if top:
        st.prefill(list(seq[:top]), 0)
    for s, n in want:
        st.save_slot(s, n)


def _state(st, d, slot, upto):
    return _slot_state(Mla, st, d, slot, upto)


def _upto(snap, n):
    return [(a[:n], b[:n]) for a, b in snap]


def _equal(a, b, where=""):
    """two results (ids, logits, slot states) of one scenario: bit for bit"""
    assert [int(x) for x in a[0]] == [int(x) for x in b[0]], ("ids", where)
    assert np.array_equal(_bits(a[1]), _bits(b[1])), ("logits", where)
    assert len(a[2]) == len(b[2])
    for x, y in zip(a[2], b[2]):
        MM._same(x, y)


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
    return ids, lg, [_state(st, d, s, p + 1) for s, p in zip(slots, pos)]


# ---- 1: on == off == decode_step on each sequence alone ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key,kv_max", [(m, KV_MAX) for m in MODELS] + [(LONG_MODEL, LONG_KV)])
def test_step_multi_equals_option_off_and_decode_step(key, kv_max):
    """rows at every edge position in one call, slots scrambled: logits and ids bit for bit, then every latent / rope-key row of every slot"""
    st, _, d = _model(*key, kv_max)
    seq, (single, snap) = _seq(*key, kv_max), _single(*key, kv_max)
    pos = POS if kv_max == KV_MAX else POS_LONG
    took = []      # not vacuous: the pass took the option's form in the on-leg and not in the off-leg (multi_path_counts)

    def counted(st):
        st.multi_path_counts(reset=True)
        out = _steps(st, d, seq, pos, kv_max=kv_max)
        took.append(st.multi_path_counts()["mla_xs_split"])
        return out

    off, on = _off_on(st, counted)
    assert took == [0, 1], ("mla_xs_split", took)
    _equal(on, off)
    for i, p in enumerate(pos):
        assert np.array_equal(_bits(on[1][i]), single[p][0]) and int(on[0][i]) == single[p][1], ("decode_step", p)
        MM._same(on[2][i], _upto(snap, p + 1))


# ---- 2: mixed passes through extend_multi -------------------------------------------------------------------------------------------------------------------
# (position of the first token, tokens): unit rows at the edges, runs across the scores-tile, stage and padding edges
MIXED = [(127, 1), (120, 10), (0, 1), (60, 70), (128, 1), (0, 2), (63, 1), (31, 1), (500, 30)]
RUNS_ONLY = [(126, 3), (30, 40), (590, 5)]
UNITS_ONLY = [(599, 1), (64, 1), (0, 1), (129, 1)]
# "multi_extend_mla_exact_mfma" takes head counts that divide 32 only (its own refusal): the other two settings run every geometry
MIXED_CASES = [(m, o) for m in MODELS for o in (None, "multi_extend_mla_exact_mfma", "multi_extend_mla_flash") if o != "multi_extend_mla_exact_mfma" or 32 % m[1] == 0]


@pytest.mark.parametrize("key,other", MIXED_CASES)
def test_mixed_passes_through_extend_multi(key, other):
    """unit rows beside runs with no run option, with "multi_extend_mla_exact_mfma" and with "multi_extend_mla_flash": on == off with the same other option; a pass
    with no unit row and a pass of unit rows only among them"""
    st, _, d = _model(*key)
    seq = _seq(*key)

    def scenario(st):
        st.create_slots(16, KV_MAX)
        ids, lgs, states, at = [], [], [], 0
        for rows in (MIXED, RUNS_ONLY, UNITS_ONLY):
            slots = SLOTS[at:at + len(rows)]
            at += len(rows)
            _fill(st, d, seq, [(s, p) for s, (p, _) in zip(slots, rows)])
            i, lg = st.extend_multi(slots, [list(seq[p:p + c]) for p, c in rows], [p for p, _ in rows], logits=True)
            ids += list(i); lgs.append(lg)
            states += [_state(st, d, s, p + c) for s, (p, c) in zip(slots, rows)]
        return ids, np.concatenate(lgs), states

    off, on = _off_on(st, scenario, **({other: 1} if other else {}))
    _equal(on, off, other)


# ---- 3: verify ----------------------------------------------------------------------------------------------------------------------------------------------
VERIFY_POS = [126, 127, 62, 30, 0]                                          # runs of 3: two rows of one run attend over different lengths of the slot, across a tile edge


@pytest.mark.parametrize("sample", [False, True])
@pytest.mark.parametrize("key", [MODELS[0], MODELS[2], MODELS[4]])
def test_verify_and_commit(key, sample):
    """verify_multi + commit_multi / verify_multi_sample: a verify with drafts from the sequence, committed as nothing; then one whose drafts are the ids the first
    returned (every draft matches), committed at different lengths: ids, n_match and the states after the commit on == off"""
    st, _, d = _model(*key)
    seq = _seq(*key)

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
        return ids, np.zeros(1, np.float32), [_state(st, d, s, p + k) for s, p, k in zip(slots, VERIFY_POS, keep)]

    off, on = _off_on(st, scenario)
    _equal(on, off, "verify + commit")


# ---- 4: generation ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lookup", [False, True])
@pytest.mark.parametrize("key", [MODELS[1], MODELS[4]])
def test_generate_multi_across_a_tile_edge(key, lookup):
    """8 tokens from positions 124 (across the second scores tile's edge), 60 (the first one's = the weighted sum's stage), 590 and 0, by generate_multi and by the
    lookup loop (steps and verify passes): tokens and end states on == off"""
    st, _, d = _model(*key)
    seq = _seq(*key)
    starts = [124, 60, 590, 0]

    def scenario(st):
        st.create_slots(16, KV_MAX)
        slots = SLOTS[:len(starts)]
        _fill(st, d, seq, list(zip(slots, starts)))
        firsts = [seq[p] for p in starts]
        if lookup:
            toks = st.generate_multi_lookup(slots, firsts, starts, 8, contexts=[list(seq[:p + 1]) for p in starts])
        else:
            toks = st.generate_multi(slots, firsts, starts, 8)
        return [x for row in toks for x in row], np.zeros(1, np.float32), [_state(st, d, s, p + 8) for s, p in zip(slots, starts)]

    off, on = _off_on(st, scenario)
    _equal(on, off, "generate")


# ---- 5: paged slots -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("page_tokens", [32, 64, 256])
@pytest.mark.parametrize("key", MODELS)
def test_paged_and_forked_slots(key, page_tokens):
    """page_tokens 32: a scores tile and a stage of the weighted sum span two pages; 64: they are a page; 256: in-page offsets reach 255.  Scrambled placement: a
    spare slot saved before the 512-token prefix and trimmed after it leaves a hole, and a page saved right behind the prefix stays held, so the page the step at
    position 512 maps does not follow the slot's others.  Then a fork at position 300 (no page edge) with the step on the dst: dst on == off, and the src's rows
    are unchanged"""
    st, _, d = _model(*key)
    seq, (single, snap) = _seq(*key), _single(*key)
    pt, far, fork_at = page_tokens, FAR, 300
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
        states = [_state(st, d, slot_of[p], p + 1) for p in POS]
        for p in others:
            st.trim_slot(slot_of[p], 0)
        st.trim_slot(dst, 0)
        st.fork_slot(slot_of[far], [dst], fork_at)
        ids2, lg2 = st.step_multi([dst], [seq[fork_at]], [fork_at], logits=True)
        states += [_state(st, d, dst, fork_at + 1), _state(st, d, slot_of[far], far + 1)]
        return list(ids) + list(ids2), np.concatenate([lg, lg2]), states

    off, on = _off_on(st, scenario)
    _equal(on, off, ("paged", pt))
    for i, p in enumerate(POS):
        assert np.array_equal(_bits(on[1][i]), single[p][0]), ("decode_step", p)
    MM._same(on[2][-1], _upto(snap, far + 1))              # the fork's src: untouched
    MM._same(on[2][-2], _upto(snap, fork_at + 1))          # the dst: the same sequence, one row behind the fork point


# ---- 6: stale scratch ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", MODELS)
def test_short_call_after_a_long_one(key):
    """a call at positions 599 and 512 leaves scores and probabilities in the scratch; the call at positions 5, 40 and 31 after it uses another row stride over
    the same bytes and is on == off: nothing beyond a row's own positions is consumed"""
    st, _, d = _model(*key)
    seq = _seq(*key)

    def scenario(st):
        st.create_slots(16, KV_MAX)
        long_pos, short_pos = [KV_MAX - 1, FAR], [5, 40, 31]
        _fill(st, d, seq, list(zip([2, 4, 1, 6, 3], long_pos + short_pos)))
        st.step_multi([2, 4], [seq[p] for p in long_pos], long_pos)
        ids, lg = st.step_multi([1, 6, 3], [seq[p] for p in short_pos], short_pos, logits=True)
        return ids, lg, [_state(st, d, s, p + 1) for s, p in zip([1, 6, 3], short_pos)]

    off, on = _off_on(st, scenario)
    _equal(on, off, "short after long")


# ---- 7: the threshold ---------------------------------------------------------------------------------------------------------------------------------------
def test_threshold_above_at_and_one():
    """with "multi_mla_exact_split_min" above every position of the call the pass keeps the one kernel; exactly at the call's longest attention, and at 1, it takes
    the split: all equal the option-off call"""
    key = MODELS[1]
    st, _, d = _model(*key)
    seq = _seq(*key)
    pos = [0, 127, 128, 300]
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
    st, _, d = _model(512, 4, False, False, kv_max=32)
    for v in (0, -5):
        with pytest.raises(ValueError) as e:
            st.set_option(MIN, v)
        assert MIN in str(e.value), str(e.value)


# ---- 8: refusals --------------------------------------------------------------------------------------------------------------------------------------------
def _calls(st, V):
    t = lambda k: [x % V for x in range(1, 1 + k)]
    return (lambda: st.step_multi([1], t(1), [0]), lambda: st.extend_multi([1], [t(3)], [0]), lambda: st.generate_multi([1], t(1), [0], 2),
            lambda: st.verify_multi([1], [t(2)], [0]), lambda: st.generate_multi_lookup([1], t(1), [0], 2))


def _refused_then_fine(st, d, state, arm, refuse, clear):
    """a slot holding a prefix (filled with nothing set); after arm() every batched call is refused by refuse(call); after clear() the slot's state -- state(slot,
    upto) -> per layer a tuple of stored arrays -- is what it was and the run succeeds"""
    st.create_slots(2, 20)
    st.reset_decode_state(d["kv_max"]); st.prefill([3, 1, 4], 0); st.save_slot(1, 3)
    before = state(1, 3)
    arm()
    for call in _calls(st, d["V"]):
        refuse(call)
    clear()
    after = state(1, 3)
    assert len(after) == len(before)
    for x, y in zip(after, before):
        assert len(x) == len(y) and all(np.array_equal(p, q) for p, q in zip(x, y))
    st.extend_multi([1], [[1, 2, 3]], [3])


def test_store_without_mla_layers_is_refused():
    from tests.test_decode_gpu import build
    from tests.test_speculative_gpu import _snap
    st, eng, orc, keep, d = build(seed=3, kv_max=32)                        # linear attention + GQA
    _stores.append(st)

    def state(slot, upto):
        st.reset_decode_state(d["kv_max"]); st.load_slot(slot, upto)
        return [tuple(x for x in row if isinstance(x, np.ndarray)) for row in _snap(st, d, upto)]

    _refused_then_fine(st, d, state, lambda: st.set_option(OPT, 1), lambda call: _state_error(call, OPT, "covers MLA layers only: this store has none"),
                       lambda: st.set_option(OPT, 0))


def test_mode_bits_stay_refused_with_their_old_text():
    st, _, d = _model(512, 4, False, False, kv_max=32)

    def arm():
        st.set_option(OPT, 1); st.set_attention_mode(True)

    _refused_then_fine(st, d, lambda s, p: _state(st, d, s, p), arm, lambda call: _state_error(call, "exact-mode only"), lambda: st.set_attention_mode(False))      # the option itself stays set
    st.set_option(OPT, 0)


# ---- 9: long slots, the flash-decode claims the unit rows ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("paged", [False, True])
def test_long_slots_under_multi_mla_fast(paged):
    """slots of 1100 positions (above mla_split_min) with "multi_mla_fast" also set, flat and in pages of 64: the rows take the split-KV flash-decode, the split has
    nothing to do, nothing is refused, and the call equals the one under that option alone -- which differs from the exact call"""
    st, _, d = _model(*LONG_MODEL, LONG_KV)
    seq = _seq(*LONG_MODEL, LONG_KV)
    pos = [1030, 40, SOFTMAX_TILE, 700]
    kw = dict(page_tokens=64, n_pages=sum(_pages(p + 1, 64) for p in pos) + 2) if paged else {}
    scenario = lambda st: _steps(st, d, seq, pos, n_slots=16, kv_max=LONG_KV, **kw)
    exact = scenario(st)
    fd, both = _off_on(st, scenario, multi_mla_fast=1)
    _equal(both, fd, "multi_mla_fast")
    assert any(not np.array_equal(_bits(fd[1][r]), _bits(exact[1][r])) for r in range(len(pos)))      # the flash-decode did run
