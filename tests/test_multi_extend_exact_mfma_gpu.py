"""The "multi_extend_exact_mfma" option (docs/design/28-multi-extend-exact-mfma.md): a run of two or more tokens entering a device slot (extend_multi /
prefill_slot) takes the exact prompt pass's three attention passes over the slot in its GQA layers -- scores and P.V on the f32 matrix cores, the exact softmax
between them.  No bit changes: every call gives what the same call gives with the option off -- ids, logits, every K / V row, every conv and recurrent state --
on flat, paged and forked slots, FP16 and E4M3 caches, whatever other rows share the pass and however the stream is cut.  There is no tolerance in this file.

The reference is never the new path: it is the same call with the option off on equally filled slots and, in test 1, also the store's own exact
prefill(run, position) (computed once per geometry and shared).  Every comparison is on ids and u32 / stored-row bit patterns."""
import functools

import numpy as np
import pytest

from tests.slots import Gqa, bits as _bits, equal, fill_prefix, off_on, options_reset, pages as _pages, slot_state, state_error, store_cache, toks as _toks

pytestmark = pytest.mark.gpu
U = np.uint32
OPT = "multi_extend_exact_mfma"
KV_MAX = 260
# (head_dim, query heads on 2 KV heads, E4M3): G = 8, 4, 2, 1, 32 -- scores tiles of 8, 16, 32, 64 and 2 tokens, P.V tiles of 4, 8, 16, 32 and 1 token
MODELS = [(256, 16, False), (128, 8, True), (64, 4, False), (64, 2, True), (64, 64, False)]
# (tokens already in the slot, tokens of the run): one tile of two rows; a run inside one 64-position tile; a run that starts on a tile edge; runs across the
# query-tile, 64-position-tile and 32-position-block edges, ends = 1 and = 33 mod 64 among them; the last one up to the slot's last position, 260
CASES = [(0, 2), (5, 63), (64, 64), (63, 130), (37, 170), (129, 131)]
SLOTS = [5, 0, 7, 2, 6, 3]                                                  # slot numbers do not follow the rows
LONGEST = 5

_stores = []
ALL_OPTS = (OPT, "multi_extend_flash", "multi_extend_la_chunk", "multi_attn_fast", "multi_attn_fast_paged")


options_off_afterwards = options_reset(_stores, ALL_OPTS)


@store_cache(_stores)
def _model(hd, nh, fp8, kv_max=KV_MAX, kinds=("gqa", "gqa")):
    """one store per geometry, built once and shared"""
    return Gqa.build(fp8, seed=3, hd=hd, nh=nh, kv_max=kv_max, kinds=list(kinds))


def _exact_run(st, d, prefix, run):
    """the single-sequence reference: prefix and run by the store's own exact prompt pass from zero state -> logits bits, id, snapshot"""
    st.reset_decode_state(d["kv_max"])
    if prefix:
        st.prefill(prefix, 0)
    tok = st.prefill(run, len(prefix))
    return dict(prefix=prefix, run=run, pos0=len(prefix), end=len(prefix) + len(run), lg=_bits(st.read_logits()), tok=tok, snap=Gqa.snap(st, d, len(prefix) + len(run)))


@functools.lru_cache(maxsize=None)
def _refs(hd, nh, fp8):
    """the six runs of CASES and their single-sequence references: computed once, shared by the tests, never modified"""
    st, _, d = _model(hd, nh, fp8)
    rng = np.random.default_rng(hd + nh)
    return [_exact_run(st, d, _toks(rng, d, p), _toks(rng, d, c)) for p, c in CASES]


# ---- 1: on == off == the single-sequence exact prompt pass --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("slot_seq", [260, 400])
@pytest.mark.parametrize("hd,nh,fp8", MODELS)
def test_runs_equal_option_off_and_single_sequence_prefill(hd, nh, fp8, slot_seq):
    """all six runs in one call, slots scrambled: logits and ids bit for bit, then every K / V row of every slot"""
    st, _, d = _model(hd, nh, fp8)
    refs = _refs(hd, nh, fp8)

    def scenario(st):
        st.create_slots(8, slot_seq)
        for ref, s in zip(refs, SLOTS):
            fill_prefix(st, d, ref["prefix"], [s])
        ids, lg = st.extend_multi(SLOTS, [r["run"] for r in refs], [r["pos0"] for r in refs], logits=True)
        return ids, lg, [slot_state(Gqa, st, d, s, r["end"]) for r, s in zip(refs, SLOTS)]

    took = []      # not vacuous: the pass took the option's form in the on-leg and not in the off-leg (multi_path_counts)

    def counted(st):
        st.multi_path_counts(reset=True)
        out = scenario(st)
        took.append(st.multi_path_counts()["gqa_xm"])
        return out

    off, on = off_on(st, OPT, counted)
    assert took == [0, 1], ("gqa_xm", took)
    equal(Gqa, on, off)
    for i, ref in enumerate(refs):
        assert np.array_equal(_bits(on[1][i]), ref["lg"]) and on[0][i] == ref["tok"], ("single-sequence prefill", i)
        Gqa.same(on[2][i], ref["snap"])


# ---- 2: cuts ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hd,nh,fp8", MODELS)
def test_cuts_give_the_bits_of_one_call(hd, nh, fp8):
    """the 170-token run as 2 + 40 + 128 tokens in three calls, as 1 + 169 (the first token by the per-row kernel), and as 64 + 64 + 42 through prefill_slot: all
    equal the run in one call (= its single-sequence reference)"""
    st, _, d = _model(hd, nh, fp8)
    ref = _refs(hd, nh, fp8)[4]
    run, p0 = ref["run"], ref["pos0"]
    st.set_option(OPT, 1)
    for cuts in ([2, 40, 128], [1, 169]):
        st.create_slots(2, KV_MAX)
        fill_prefix(st, d, ref["prefix"], [1])
        at = 0
        for c in cuts:
            ids, lg = st.extend_multi([1], [run[at:at + c]], [p0 + at], logits=True)
            at += c
        assert np.array_equal(_bits(lg[0]), ref["lg"]) and ids[0] == ref["tok"], cuts
        Gqa.same(slot_state(Gqa, st, d, 1, ref["end"]), ref["snap"])
    st.create_slots(2, KV_MAX)
    fill_prefix(st, d, ref["prefix"], [1])
    tok = st.prefill_slot(1, run, p0, chunk=64)
    st.set_option(OPT, 0)
    assert tok == ref["tok"]
    Gqa.same(slot_state(Gqa, st, d, 1, ref["end"]), ref["snap"])


# ---- 3: mixed passes ----------------------------------------------------------------------------------------------------------------------------------------
def _mixed(st, d, refs, rows, slot_seq=KV_MAX, **slots_kw):
    """rows = [("u" | "r", case)]: a unit row consumes the first token of the case's run behind its prefix, a run row the whole run -> (ids, logits, states)"""
    st.create_slots(8, slot_seq, **slots_kw)
    slots = list(range(1, 1 + len(rows)))
    for (kind, i), s in zip(rows, slots):
        fill_prefix(st, d, refs[i]["prefix"], [s])
    ids, lg = st.extend_multi(slots, [refs[i]["run"][:1] if k == "u" else refs[i]["run"] for k, i in rows], [refs[i]["pos0"] for _, i in rows], logits=True)
    return ids, lg, [slot_state(Gqa, st, d, s, refs[i]["pos0"] + (1 if k == "u" else len(refs[i]["run"]))) for (k, i), s in zip(rows, slots)]


@pytest.mark.parametrize("hd,nh,fp8", MODELS)
def test_mixed_passes(hd, nh, fp8):
    """decode rows and prompt chunks in one pass, unit rows longer (position 129) and shorter (0, 5) than the runs; a pass with no unit row; a pass of unit rows
    only: every row on == off"""
    st, _, d = _model(hd, nh, fp8)
    refs = _refs(hd, nh, fp8)
    for rows in ([("u", 5), ("r", 1), ("u", 0), ("u", 1), ("r", 3)], [("r", 2), ("r", 0), ("r", 4)]):
        off, on = off_on(st, OPT, lambda st: _mixed(st, d, refs, rows))
        equal(Gqa, on, off, rows)

    def steps(st):
        st.create_slots(8, KV_MAX)
        pick, slots = [1, 3, 5], [3, 0, 5]
        for i, s in zip(pick, slots):
            fill_prefix(st, d, refs[i]["prefix"], [s])
        ids, lg = st.step_multi(slots, [refs[i]["run"][0] for i in pick], [refs[i]["pos0"] for i in pick], logits=True)
        return ids, lg, [slot_state(Gqa, st, d, s, refs[i]["pos0"] + 1) for i, s in zip(pick, slots)]

    off, on = off_on(st, OPT, steps)
    equal(Gqa, on, off, "step_multi")


def test_verify_and_commit_are_untouched():
    st, _, d = _model(64, 4, False)
    refs = _refs(64, 4, False)

    def scenario(st):
        st.create_slots(8, KV_MAX)
        pick, slots = [1, 2, 3], [3, 0, 5]
        for i, s in zip(pick, slots):
            fill_prefix(st, d, refs[i]["prefix"], [s])
        pos = [refs[i]["pos0"] for i in pick]
        drafts = [refs[i]["run"][:3] for i in pick]
        greedy, nm = st.verify_multi(slots, drafts, pos)
        keep = [min(m + 1, 2) for m in nm]
        st.commit_multi(keep)
        return [g for row in greedy for g in row] + list(nm), np.zeros(1, np.float32), [slot_state(Gqa, st, d, s, p + k) for s, p, k in zip(slots, pos, keep)]

    off, on = off_on(st, OPT, scenario)
    equal(Gqa, on, off, "verify + commit")


# ---- 4: paged slots -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("page_tokens", [32, 64, 256])
@pytest.mark.parametrize("hd,nh,fp8", MODELS)
def test_paged_and_forked_slots(hd, nh, fp8, page_tokens):
    """page_tokens 32: a 64-position tile spans two pages; 64: a tile is a page; 256: in-page offsets reach 255.  Scrambled placement: a spare slot saved before
    the longest run's prefix and trimmed after it leaves a hole, and a page saved right behind the prefix stays held, so that run's pages are not consecutive.
    Then a fork at position 129 (no page edge) with the run entering the dst: dst on == off, and the src's rows are unchanged"""
    st, _, d = _model(hd, nh, fp8)
    refs = _refs(hd, nh, fp8)
    pt = page_tokens
    ref = refs[LONGEST]

    def scenario(st):
        spare, dst = 1, 4
        need = sum(_pages(r["end"], pt) for r in refs) + 2 * _pages(ref["end"], pt)
        st.create_slots(8, KV_MAX, page_tokens=pt, n_pages=need + 2)
        for r, s in list(zip(refs, SLOTS))[:LONGEST]:
            fill_prefix(st, d, r["prefix"], [s])
        st.reset_decode_state(d["kv_max"]); st.save_slot(spare, min(100, pt))
        fill_prefix(st, d, ref["prefix"], [SLOTS[LONGEST]])
        st.reset_decode_state(d["kv_max"]); st.save_slot(dst, 1)
        st.trim_slot(spare, 0)
        ids, lg = st.extend_multi(SLOTS, [r["run"] for r in refs], [r["pos0"] for r in refs], logits=True)
        used = [int(x) for x in st.slot_page_ids(SLOTS[LONGEST])[0][:_pages(ref["end"], pt)]]
        assert min(used) >= 0 and used != list(range(used[0], used[0] + len(used))), ("the longest run's pages are consecutive", used)
        states = [slot_state(Gqa, st, d, s, r["end"]) for r, s in zip(refs, SLOTS)]
        for s in SLOTS[:LONGEST]:
            st.trim_slot(s, 0)
        st.trim_slot(dst, 0)
        st.trim_slot(SLOTS[LONGEST], ref["pos0"])
        st.fork_slot(SLOTS[LONGEST], [dst], ref["pos0"])
        ids2, lg2 = st.extend_multi([dst], [ref["run"]], [ref["pos0"]], logits=True)
        states += [slot_state(Gqa, st, d, dst, ref["end"]), slot_state(Gqa, st, d, SLOTS[LONGEST], ref["pos0"])]
        return list(ids) + list(ids2), np.concatenate([lg, lg2]), states

    off, on = off_on(st, OPT, scenario)
    equal(Gqa, on, off, ("paged", pt))
    Gqa.same(on[2][-1], [(k, li, a[:ref["pos0"]], b[:ref["pos0"]]) for k, li, a, b in ref["snap"]])      # the fork's src: untouched
    Gqa.same(on[2][-2], ref["snap"])


# ---- 5: a hybrid store --------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fp8", [False, True])
def test_hybrid_store_and_the_chunked_delta_rule(fp8):
    """linear attention + GQA: on == off including conv and recurrent state; with "multi_extend_la_chunk" also set and runs of >= 64 tokens, both options ==
    "multi_extend_la_chunk" alone"""
    st, _, d = _model(64, 4, fp8, kinds=("la", "gqa", "la", "gqa"))
    rng = np.random.default_rng(21)
    prefixes, runs = [_toks(rng, d, 37), _toks(rng, d, 5), _toks(rng, d, 64)], [_toks(rng, d, 170), _toks(rng, d, 1), _toks(rng, d, 70)]

    def scenario(st):
        st.create_slots(4, KV_MAX)
        slots = [2, 0, 3]
        for p, s in zip(prefixes, slots):
            fill_prefix(st, d, p, [s])
        ids, lg = st.extend_multi(slots, runs, [len(p) for p in prefixes], logits=True)
        ids2, lg2 = st.step_multi(slots, list(ids), [len(p) + len(r) for p, r in zip(prefixes, runs)], logits=True)
        return list(ids) + list(ids2), np.concatenate([lg, lg2]), [slot_state(Gqa, st, d, s, len(p) + len(r) + 1) for s, p, r in zip(slots, prefixes, runs)]

    off, on = off_on(st, OPT, scenario)
    equal(Gqa, on, off, "hybrid")
    lc, both = off_on(st, OPT, scenario, multi_extend_la_chunk=1)
    equal(Gqa, both, lc, "hybrid + multi_extend_la_chunk")


# ---- 6: long slots, flash-decode unit rows ------------------------------------------------------------------------------------------------------------------
LONG_KV = 1100


@pytest.mark.parametrize("paged", [False, True])
def test_long_slots_with_flash_decode_unit_rows(paged):
    """slots of 1100 positions (above gqa_split_min) with "multi_attn_fast" (flat) / "multi_attn_fast_paged" (pages of 64) also set: the unit rows take the
    split-KV flash-decode and equal the call under that option alone; the runs equal the call with every option off"""
    st, _, d = _model(128, 8, True, kv_max=LONG_KV)
    rng = np.random.default_rng(77)
    cases = [(1030, 1), (900, 130), (40, 1), (700, 2), (1050, 50)]
    prefixes = [_toks(rng, d, p) for p, _ in cases]
    runs = [_toks(rng, d, c) for _, c in cases]
    slots = [4, 1, 0, 3, 2]
    kw = dict(page_tokens=64, n_pages=sum(_pages(p + c, 64) for p, c in cases) + 2) if paged else {}
    fast = "multi_attn_fast_paged" if paged else "multi_attn_fast"

    def scenario(st):
        st.create_slots(5, LONG_KV, **kw)
        for p, s in zip(prefixes, slots):
            fill_prefix(st, d, p, [s])
        ids, lg = st.extend_multi(slots, runs, [p for p, _ in cases], logits=True)
        return ids, lg, [slot_state(Gqa, st, d, s, p + c) for s, (p, c) in zip(slots, cases)]

    exact = scenario(st)                                                    # every option off
    fd, both = off_on(st, OPT, scenario, **{fast: 1})
    for r, (p, c) in enumerate(cases):
        want = fd if c == 1 else exact
        assert both[0][r] == want[0][r] and np.array_equal(_bits(both[1][r]), _bits(want[1][r])), ("row", r, "unit" if c == 1 else "run")
        Gqa.same(both[2][r], want[2][r])
    assert any(not np.array_equal(_bits(fd[1][r]), _bits(exact[1][r])) for r, (_, c) in enumerate(cases) if c == 1)      # the flash-decode did run on the unit rows


# ---- 7: stale scratch ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hd,nh,fp8", MODELS)
def test_short_call_after_a_long_one(hd, nh, fp8):
    """a long call leaves scores, exponentials, row maxima and sums in the scratch; the short call after it uses another row stride over the same bytes and is
    on == off: masked score positions are never consumed"""
    st, _, d = _model(hd, nh, fp8)
    refs = _refs(hd, nh, fp8)

    def scenario(st):
        st.create_slots(8, KV_MAX)
        for i, s in zip([5, 3, 1, 0], [2, 4, 1, 6]):
            fill_prefix(st, d, refs[i]["prefix"], [s])
        st.extend_multi([2, 4], [refs[5]["run"], refs[3]["run"]], [refs[5]["pos0"], refs[3]["pos0"]])
        ids, lg = st.extend_multi([1, 6], [refs[1]["run"][:7], refs[0]["run"]], [refs[1]["pos0"], refs[0]["pos0"]], logits=True)
        return ids, lg, [slot_state(Gqa, st, d, 1, refs[1]["pos0"] + 7), slot_state(Gqa, st, d, 6, refs[0]["end"])]

    off, on = off_on(st, OPT, scenario)
    equal(Gqa, on, off, "short after long")


# ---- 8: refusals --------------------------------------------------------------------------------------------------------------------------------------------
def _calls(st, V):
    t = lambda k: [x % V for x in range(1, 1 + k)]
    return (lambda: st.step_multi([1], t(1), [0]), lambda: st.extend_multi([1], [t(3)], [0]), lambda: st.generate_multi([1], t(1), [0], 2),
            lambda: st.verify_multi([1], [t(2)], [0]), lambda: st.generate_multi_lookup([1], t(1), [0], 2))


def _refused_then_fine(st, d, arm, refuse, clear):
    """a slot holding a prefix (filled with nothing set); after arm() every batched call is refused by refuse(call); after clear() the slot's state is what it was
    and the run succeeds"""
    st.create_slots(2, 20)
    fill_prefix(st, d, [3, 1, 4], [1])
    before = slot_state(Gqa, st, d, 1, 3)
    arm()
    for call in _calls(st, d["V"]):
        refuse(call)
    clear()
    Gqa.same(slot_state(Gqa, st, d, 1, 3), before)
    st.extend_multi([1], [[1, 2, 3]], [3])


def test_both_run_options_are_refused():
    st, _, d = _model(64, 4, False, kv_max=32)

    def arm():
        st.set_option(OPT, 1); st.set_option("multi_extend_flash", 1)

    _refused_then_fine(st, d, arm, lambda call: state_error(call, OPT, "multi_extend_flash"), lambda: st.set_option("multi_extend_flash", 0))      # the option itself stays set
    st.set_option(OPT, 0)


def test_store_without_gqa_layers_is_refused():
    st, _, d = _model(64, 4, False, kv_max=32, kinds=("la", "la"))
    _refused_then_fine(st, d, lambda: st.set_option(OPT, 1), lambda call: state_error(call, OPT, "has none"), lambda: st.set_option(OPT, 0))


def test_group_of_three_heads_is_refused_not_run_by_the_per_row_kernel():
    st, _, d = _model(64, 6, False, kv_max=32)
    st.create_slots(2, 20)
    want = st.extend_multi([1], [[1, 2, 3]], [0], logits=True)              # succeeds with the option off

    def refuse(call):
        with pytest.raises(ValueError) as e:
            call()
        assert OPT in str(e.value) and "divide 32" in str(e.value), str(e.value)

    _refused_then_fine(st, d, lambda: st.set_option(OPT, 1), refuse, lambda: st.set_option(OPT, 0))
    st.create_slots(2, 20)
    got = st.extend_multi([1], [[1, 2, 3]], [0], logits=True)
    assert got[0] == want[0] and np.array_equal(_bits(got[1]), _bits(want[1]))


def test_mode_bits_stay_refused_with_their_old_text():
    st, _, d = _model(64, 4, False, kv_max=32)

    def arm():
        st.set_option(OPT, 1); st.set_attention_mode(True)

    _refused_then_fine(st, d, arm, lambda call: state_error(call, "exact-mode only"), lambda: st.set_attention_mode(False))      # the option itself stays set
    st.set_option(OPT, 0)
