"""The "multi_extend_mla_exact_mfma" option (docs/design/29-multi-extend-mla-exact-mfma.md): a run of two or more tokens entering a device slot (extend_multi /
prefill_slot) takes the exact MLA prompt pass's three attention passes over the slot's latent and rope-key rows in its MLA layers -- the two score dots and P.V
on the f32 matrix cores, the exact softmax between them.  No bit changes: every call gives what the same call gives with the option off -- ids, logits, every
latent and rope-key row -- on flat, paged and forked slots, FP16 and E4M3 caches, kv_lora_rank 512 / 256, the direct and the LoRA query path, whatever other
rows share the pass and however the stream is cut.  There is no tolerance in this file.

The reference is never the new path: it is the same call with the option off on equally filled slots and, in test 1, also the store's own exact
prefill(run, position) from zero state (computed once per geometry and shared).  Every comparison is on ids and u32 / stored-row bit patterns."""
import functools

import numpy as np
import pytest

import tests.test_multi_mla_gpu as MM
from tests.test_multi_paged_gpu import Mla, _slot_state, _state_error

pytestmark = pytest.mark.gpu
U = np.uint32
OPT = "multi_extend_mla_exact_mfma"
KV_MAX = 260
# (kv_lora_rank, heads, LoRA query path, E4M3 caches): scores tiles of 16, 32, 4, 2 and 64 tokens, P.V tiles of 8, 16, 2, 1 and 32 tokens
MODELS = [(512, 4, False, False), (256, 2, False, True), (512, 16, True, True), (512, 32, False, False), (256, 1, False, False)]
# (tokens already in the slot, tokens of the run): one tile of two rows; a run inside one 64-position tile; a run that starts on a tile edge; runs across the
# query-tile, 64-position-tile and 32-position-block edges; the last one up to the slot's last position, 260
CASES = [(0, 2), (5, 63), (64, 64), (63, 130), (37, 170), (129, 131)]
SLOTS = [5, 0, 7, 2, 6, 3]                                                  # slot numbers do not follow the rows
LONGEST = 5
R170 = 4

_stores = []
ALL_OPTS = (OPT, "multi_extend_mla_flash", "multi_mla_fast", "multi_extend_exact_mfma", "multi_extend_la_chunk")


@pytest.fixture(autouse=True)
def options_off_afterwards():
    yield
    for st in _stores:
        for o in ALL_OPTS:
            st.set_option(o, 0)
        st.set_attention_mode(False)


def _toks(rng, d, n):
    return [int(x) for x in rng.integers(0, d["V"], n)]


def _bits(x):
    return np.ascontiguousarray(x).view(U).copy()


def _pages(n, pt):
    return (n + pt - 1) // pt


@functools.lru_cache(maxsize=None)
def _model(klr, nh, lora, fp8, kv_max=KV_MAX):
    """one store per geometry, built once and shared"""
    st, eng, keep, d = MM._build(fp8, seed=3, klr=klr, nh=nh, lora=lora, kv_max=kv_max)
    _stores.append(st)
    return st, (eng, keep), d


def _exact_run(st, d, prefix, run):
    """the single-sequence reference: prefix and run by the store's own exact prompt pass from zero state -> logits bits, id, snapshot"""
    MM._start(st, d, prefix)
    tok = st.prefill(run, len(prefix))
    return dict(prefix=prefix, run=run, pos0=len(prefix), end=len(prefix) + len(run), lg=_bits(st.read_logits()), tok=tok, snap=MM._snap(st, d, len(prefix) + len(run)))


@functools.lru_cache(maxsize=None)
def _refs(klr, nh, lora, fp8):
    """the six runs of CASES and their single-sequence references: computed once, shared by the tests, never modified"""
    st, _, d = _model(klr, nh, lora, fp8)
    rng = np.random.default_rng(klr + nh)
    return [_exact_run(st, d, _toks(rng, d, p), _toks(rng, d, c)) for p, c in CASES]


def _fill(st, d, prefix, slots):
    """the prefix, by the exact prompt pass on the store's own sequence, into every slot of `slots`"""
    MM._start(st, d, prefix)
    for s in slots:
        st.save_slot(s, len(prefix))


def _state(st, d, slot, upto):
    return _slot_state(Mla, st, d, slot, upto)


def _equal(a, b, where=""):
    """two results (ids, logits, slot states) of one scenario: bit for bit"""
    assert list(a[0]) == list(b[0]), ("ids", where)
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


# ---- 1: on == off == the single-sequence exact prompt pass --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("slot_seq", [260, 400])
@pytest.mark.parametrize("key", MODELS)
def test_runs_equal_option_off_and_single_sequence_prefill(key, slot_seq):
    """all six runs in one call, slots scrambled: logits and ids bit for bit, then every latent / rope-key row of every slot"""
    st, _, d = _model(*key)
    refs = _refs(*key)

    def scenario(st):
        st.create_slots(8, slot_seq)
        for ref, s in zip(refs, SLOTS):
            _fill(st, d, ref["prefix"], [s])
        ids, lg = st.extend_multi(SLOTS, [r["run"] for r in refs], [r["pos0"] for r in refs], logits=True)
        return ids, lg, [_state(st, d, s, r["end"]) for r, s in zip(refs, SLOTS)]

    took = []      # not vacuous: the pass took the option's form in the on-leg and not in the off-leg (multi_path_counts)

    def counted(st):
        st.multi_path_counts(reset=True)
        out = scenario(st)
        took.append(st.multi_path_counts()["mla_xm"])
        return out

    off, on = _off_on(st, counted)
    assert took == [0, 1], ("mla_xm", took)
    _equal(on, off)
    for i, ref in enumerate(refs):
        assert np.array_equal(_bits(on[1][i]), ref["lg"]) and on[0][i] == ref["tok"], ("single-sequence prefill", i)
        MM._same(on[2][i], ref["snap"])


# ---- 2: cuts ------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", MODELS)
def test_cuts_give_the_bits_of_one_call(key):
    """the 170-token run as 2 + 40 + 128 tokens in three calls, as 1 + 169 (the first token by the per-row kernel), and as 64 + 64 + 42 through prefill_slot: all
    equal the run in one call (= its single-sequence reference)"""
    st, _, d = _model(*key)
    ref = _refs(*key)[R170]
    run, p0 = ref["run"], ref["pos0"]
    st.set_option(OPT, 1)
    for cuts in ([2, 40, 128], [1, 169]):
        st.create_slots(2, KV_MAX)
        _fill(st, d, ref["prefix"], [1])
        at = 0
        for c in cuts:
            ids, lg = st.extend_multi([1], [run[at:at + c]], [p0 + at], logits=True)
            at += c
        assert np.array_equal(_bits(lg[0]), ref["lg"]) and ids[0] == ref["tok"], cuts
        MM._same(_state(st, d, 1, ref["end"]), ref["snap"])
    st.create_slots(2, KV_MAX)
    _fill(st, d, ref["prefix"], [1])
    tok = st.prefill_slot(1, run, p0, chunk=64)
    st.set_option(OPT, 0)
    assert tok == ref["tok"]
    MM._same(_state(st, d, 1, ref["end"]), ref["snap"])


# ---- 3: mixed passes ----------------------------------------------------------------------------------------------------------------------------------------
def _mixed(st, d, refs, rows, slot_seq=KV_MAX, **slots_kw):
    """rows = [("u" | "r", case)]: a unit row consumes the first token of the case's run behind its prefix, a run row the whole run -> (ids, logits, states)"""
    st.create_slots(8, slot_seq, **slots_kw)
    slots = list(range(1, 1 + len(rows)))
    for (kind, i), s in zip(rows, slots):
        _fill(st, d, refs[i]["prefix"], [s])
    ids, lg = st.extend_multi(slots, [refs[i]["run"][:1] if k == "u" else refs[i]["run"] for k, i in rows], [refs[i]["pos0"] for _, i in rows], logits=True)
    return ids, lg, [_state(st, d, s, refs[i]["pos0"] + (1 if k == "u" else len(refs[i]["run"]))) for (k, i), s in zip(rows, slots)]


@pytest.mark.parametrize("key", MODELS)
def test_mixed_passes(key):
    """decode rows and prompt chunks in one pass, unit rows longer (position 129) and shorter (0, 5) than the runs; a pass with no unit row; a pass of unit rows
    only: every row on == off"""
    st, _, d = _model(*key)
    refs = _refs(*key)
    for rows in ([("u", 5), ("r", 1), ("u", 0), ("u", 1), ("r", 3)], [("r", 2), ("r", 0), ("r", 4)]):
        off, on = _off_on(st, lambda st: _mixed(st, d, refs, rows))
        _equal(on, off, rows)

    def steps(st):
        st.create_slots(8, KV_MAX)
        pick, slots = [1, 3, 5], [3, 0, 5]
        for i, s in zip(pick, slots):
            _fill(st, d, refs[i]["prefix"], [s])
        ids, lg = st.step_multi(slots, [refs[i]["run"][0] for i in pick], [refs[i]["pos0"] for i in pick], logits=True)
        return ids, lg, [_state(st, d, s, refs[i]["pos0"] + 1) for i, s in zip(pick, slots)]

    off, on = _off_on(st, steps)
    _equal(on, off, "step_multi")


def test_verify_and_commit_are_untouched():
    key = MODELS[0]
    st, _, d = _model(*key)
    refs = _refs(*key)

    def scenario(st):
        st.create_slots(8, KV_MAX)
        pick, slots = [1, 2, 3], [3, 0, 5]
        for i, s in zip(pick, slots):
            _fill(st, d, refs[i]["prefix"], [s])
        pos = [refs[i]["pos0"] for i in pick]
        drafts = [refs[i]["run"][:3] for i in pick]
        greedy, nm = st.verify_multi(slots, drafts, pos)
        keep = [min(m + 1, 2) for m in nm]
        st.commit_multi(keep)
        return [g for row in greedy for g in row] + list(nm), np.zeros(1, np.float32), [_state(st, d, s, p + k) for s, p, k in zip(slots, pos, keep)]

    off, on = _off_on(st, scenario)
    _equal(on, off, "verify + commit")


# ---- 4: paged and forked slots ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("page_tokens", [32, 64, 256])
@pytest.mark.parametrize("key", MODELS)
def test_paged_and_forked_slots(key, page_tokens):
    """page_tokens 32: a 64-position tile spans two pages; 64: a tile is a page; 256: in-page offsets reach 255.  Scrambled placement: a spare slot saved before
    the longest run's prefix and trimmed after it leaves a hole, and a page saved right behind the prefix stays held, so that run's pages are not consecutive.
    Then a fork at position 129 (no page edge) with the run entering the dst: dst on == off, and the src's rows are unchanged"""
    st, _, d = _model(*key)
    refs = _refs(*key)
    pt = page_tokens
    ref = refs[LONGEST]

    def scenario(st):
        spare, dst = 1, 4
        need = sum(_pages(r["end"], pt) for r in refs) + 2 * _pages(ref["end"], pt)
        st.create_slots(8, KV_MAX, page_tokens=pt, n_pages=need + 2)
        for r, s in list(zip(refs, SLOTS))[:LONGEST]:
            _fill(st, d, r["prefix"], [s])
        st.reset_decode_state(d["kv_max"]); st.save_slot(spare, min(100, pt))
        _fill(st, d, ref["prefix"], [SLOTS[LONGEST]])
        st.reset_decode_state(d["kv_max"]); st.save_slot(dst, 1)
        st.trim_slot(spare, 0)
        ids, lg = st.extend_multi(SLOTS, [r["run"] for r in refs], [r["pos0"] for r in refs], logits=True)
        used = [int(x) for x in st.slot_page_ids(SLOTS[LONGEST])[0][:_pages(ref["end"], pt)]]
        assert min(used) >= 0 and used != list(range(used[0], used[0] + len(used))), ("the longest run's pages are consecutive", used)
        states = [_state(st, d, s, r["end"]) for r, s in zip(refs, SLOTS)]
        for s in SLOTS[:LONGEST]:
            st.trim_slot(s, 0)
        st.trim_slot(dst, 0)
        st.trim_slot(SLOTS[LONGEST], ref["pos0"])
        st.fork_slot(SLOTS[LONGEST], [dst], ref["pos0"])
        ids2, lg2 = st.extend_multi([dst], [ref["run"]], [ref["pos0"]], logits=True)
        states += [_state(st, d, dst, ref["end"]), _state(st, d, SLOTS[LONGEST], ref["pos0"])]
        return list(ids) + list(ids2), np.concatenate([lg, lg2]), states

    off, on = _off_on(st, scenario)
    _equal(on, off, ("paged", pt))
    MM._same(on[2][-1], [(a[:ref["pos0"]], b[:ref["pos0"]]) for a, b in ref["snap"]])      # the fork's src: untouched
    MM._same(on[2][-2], ref["snap"])


# ---- 5: long slots, flash-decode unit rows ------------------------------------------------------------------------------------------------------------------
LONG_KV = 1100
LONG_KEY = (512, 4, False, True)


@pytest.mark.parametrize("paged", [False, True])
def test_long_slots_with_flash_decode_unit_rows(paged):
    """slots of 1100 positions (above mla_split_min) with "multi_mla_fast" also set, flat and in pages of 64: the unit rows take the split-KV flash-decode and
    equal the call under that option alone; the runs equal the call with every option off"""
    st, _, d = _model(*LONG_KEY, kv_max=LONG_KV)
    rng = np.random.default_rng(77)
    cases = [(1030, 1), (900, 130), (40, 1), (700, 2), (1050, 50)]
    prefixes = [_toks(rng, d, p) for p, _ in cases]
    runs = [_toks(rng, d, c) for _, c in cases]
    slots = [4, 1, 0, 3, 2]
    kw = dict(page_tokens=64, n_pages=sum(_pages(p + c, 64) for p, c in cases) + 2) if paged else {}

    def scenario(st):
        st.create_slots(5, LONG_KV, **kw)
        for p, s in zip(prefixes, slots):
            _fill(st, d, p, [s])
        ids, lg = st.extend_multi(slots, runs, [p for p, _ in cases], logits=True)
        return ids, lg, [_state(st, d, s, p + c) for s, (p, c) in zip(slots, cases)]

    exact = scenario(st)                                                    # every option off
    fd, both = _off_on(st, scenario, multi_mla_fast=1)
    for r, (p, c) in enumerate(cases):
        want = fd if c == 1 else exact
        assert both[0][r] == want[0][r] and np.array_equal(_bits(both[1][r]), _bits(want[1][r])), ("row", r, "unit" if c == 1 else "run")
        MM._same(both[2][r], want[2][r])
    assert any(not np.array_equal(_bits(fd[1][r]), _bits(exact[1][r])) for r, (_, c) in enumerate(cases) if c == 1)      # the flash-decode did run on the unit rows


# ---- 6: stale scratch ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", MODELS)
def test_short_call_after_a_long_one(key):
    """a long call leaves scores, exponentials, row maxima and sums in the scratch; the short call after it uses another row stride over the same bytes and is
    on == off: masked score positions are never consumed"""
    st, _, d = _model(*key)
    refs = _refs(*key)

    def scenario(st):
        st.create_slots(8, KV_MAX)
        for i, s in zip([5, 3, 1, 0], [2, 4, 1, 6]):
            _fill(st, d, refs[i]["prefix"], [s])
        st.extend_multi([2, 4], [refs[5]["run"], refs[3]["run"]], [refs[5]["pos0"], refs[3]["pos0"]])
        ids, lg = st.extend_multi([1, 6], [refs[1]["run"][:7], refs[0]["run"]], [refs[1]["pos0"], refs[0]["pos0"]], logits=True)
        return ids, lg, [_state(st, d, 1, refs[1]["pos0"] + 7), _state(st, d, 6, refs[0]["end"])]

    off, on = _off_on(st, scenario)
    _equal(on, off, "short after long")


# ---- 7: refusals --------------------------------------------------------------------------------------------------------------------------------------------
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


def test_both_mla_run_options_are_refused():
    st, _, d = _model(512, 4, False, False, kv_max=32)

    def arm():
        st.set_option(OPT, 1); st.set_option("multi_extend_mla_flash", 1)

    _refused_then_fine(st, d, lambda s, p: _state(st, d, s, p), arm, lambda call: _state_error(call, OPT, "multi_extend_mla_flash"),
                       lambda: st.set_option("multi_extend_mla_flash", 0))      # the option itself stays set
    st.set_option(OPT, 0)


def test_store_without_mla_layers_is_refused():
    from tests.test_decode_gpu import build
    from tests.test_speculative_gpu import _snap
    st, eng, orc, keep, d = build(seed=3, kv_max=32)                        # linear attention + GQA
    _stores.append(st)

    def state(slot, upto):
        st.reset_decode_state(d["kv_max"]); st.load_slot(slot, upto)
        return [tuple(x for x in row if isinstance(x, np.ndarray)) for row in _snap(st, d, upto)]

    _refused_then_fine(st, d, state, lambda: st.set_option(OPT, 1), lambda call: _state_error(call, OPT, "has none"), lambda: st.set_option(OPT, 0))


def test_three_heads_are_refused_not_run_by_the_per_row_kernel():
    st, _, d = _model(512, 3, False, False, kv_max=32)
    st.create_slots(2, 20)
    want = st.extend_multi([1], [[1, 2, 3]], [0], logits=True)              # succeeds with the option off

    def refuse(call):
        with pytest.raises(ValueError) as e:
            call()
        assert OPT in str(e.value) and "divide 32" in str(e.value), str(e.value)

    _refused_then_fine(st, d, lambda s, p: _state(st, d, s, p), lambda: st.set_option(OPT, 1), refuse, lambda: st.set_option(OPT, 0))
    st.create_slots(2, 20)
    got = st.extend_multi([1], [[1, 2, 3]], [0], logits=True)
    assert got[0] == want[0] and np.array_equal(_bits(got[1]), _bits(want[1]))


def test_mode_bits_stay_refused_with_their_old_text():
    st, _, d = _model(512, 4, False, False, kv_max=32)

    def arm():
        st.set_option(OPT, 1); st.set_attention_mode(True)

    _refused_then_fine(st, d, lambda s, p: _state(st, d, s, p), arm, lambda call: _state_error(call, "exact-mode only"), lambda: st.set_attention_mode(False))      # the option itself stays set
    st.set_option(OPT, 0)
