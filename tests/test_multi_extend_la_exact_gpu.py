"""The "multi_extend_la_exact" option (docs/design/36-multi-extend-la-exact.md): a run of "multi_extend_la_exact_min" or more tokens entering a device slot
(extend_multi / prefill_slot) takes the staged form of the exact prompt pass in its linear-attention layers.  No bit may change: every call gives the ids, the
logits and the slot state (conv inputs, recurrent state, K / V rows) it gives with the option off, and what the single-sequence exact prefill / decode_step give
on the store's own sequence -- whatever rows share the pass, however the stream is cut, on flat, paged and forked slots, with FP16 and E4M3 caches.

The references are never the path under test: the same call with the option off, and the store's own exact prompt pass (computed once per model and shared).
Every comparison is on ids and u32 / stored-row bit patterns."""
import functools

import numpy as np
import pytest

from tests.test_decode_gpu import build
from tests.test_multi_paged_gpu import _state_error
from tests.test_speculative_gpu import _same, _snap

pytestmark = pytest.mark.gpu
U = np.uint32
OPT, MIN = "multi_extend_la_exact", "multi_extend_la_exact_min"
CHUNK, XM = "multi_extend_la_chunk", "multi_extend_exact_mfma"
KV_MAX = 260
LA = ("la", "la")
HYBRID = ("la", "gqa", "la")
# (kinds, (key heads, value heads), (dk, dv), E4M3 KV): 1, 2 and 4 value heads per key head; both key widths; dv > dk; a GQA layer between, both cache types
MODELS = [(LA, (2, 4), (128, 128), False), (LA, (1, 8), (128, 128), False), (LA, (4, 16), (128, 128), False), (LA, (2, 4), (64, 64), False), (LA, (2, 4), (64, 128), False),
          (HYBRID, (2, 4), (128, 128), False), (HYBRID, (2, 4), (128, 128), True)]
IDS = ["la-2x4", "la-1x8", "la-4x16", "la-dk64", "la-dk64-dv128", "hybrid-fp16", "hybrid-e4m3"]
# (tokens already in the slot, tokens of the run): shorter than the DMA ring's look-ahead; the ring's edges; the 16-token conv tile's edge; longer runs
CASES = [(0, 2), (5, 3), (0, 4), (3, 5), (37, 16), (5, 17), (2, 33), (37, 170)]

_stores = []


@pytest.fixture(autouse=True)
def options_off_afterwards():
    yield
    for st in _stores:
        st.set_option(OPT, 0); st.set_option(MIN, 8); st.set_option(CHUNK, 0); st.set_option(XM, 0); st.set_option("multi_attn_fast", 0)
        st.set_attention_mode(False); st.set_prefill_chunk(0)


def _toks(rng, d, n):
    return [int(x) for x in rng.integers(0, d["V"], n)]


def _bits(x):
    return np.ascontiguousarray(x).view(U).copy()


@functools.lru_cache(maxsize=None)
def _model(kinds, la_heads=(2, 4), la_dkdv=(128, 128), fp8=False, kv_max=KV_MAX):
    """one store per model, built once and shared"""
    st, eng, orc, keep, d = build(seed=3, hd=64, nh=4, kv_max=kv_max, kinds=list(kinds), la_heads=la_heads, la_dkdv=la_dkdv)
    if fp8:
        st.set_kv_dtype(True); d["fp8"] = True
    _stores.append(st)
    return st, (eng, orc, keep), d


def _exact_run(st, d, prefix, run):
    """the single-sequence reference: prefix and run by the store's own exact prompt pass from zero state -> logits bits, id, snapshot"""
    st.reset_decode_state(d["kv_max"])
    if prefix:
        st.prefill(prefix, 0)
    tok = st.prefill(run, len(prefix))
    return dict(prefix=prefix, run=run, pos0=len(prefix), end=len(prefix) + len(run), lg=_bits(st.read_logits()), tok=tok, snap=_snap(st, d, len(prefix) + len(run)))


@functools.lru_cache(maxsize=None)
def _refs(model):
    """the runs of CASES and their single-sequence references: computed once per model, shared by the tests, never modified"""
    st, _, d = _model(*model)
    rng = np.random.default_rng(7 + model[1][1])
    return [_exact_run(st, d, _toks(rng, d, p), _toks(rng, d, c)) for p, c in CASES]


def _fill(st, d, prefix, slots):
    """the prefix, by the exact prompt pass on the store's own sequence, into every slot of `slots`"""
    st.reset_decode_state(d["kv_max"])
    if prefix:
        st.prefill(prefix, 0)
    for s in slots:
        st.save_slot(s, len(prefix))


def _slot_state(st, d, slot, upto):
    st.reset_decode_state(d["kv_max"])
    st.load_slot(slot, upto)
    return _snap(st, d, upto)


def _assert_run(st, d, ref, slot, tok, lg, where=""):
    assert np.array_equal(_bits(lg), ref["lg"]), ("logits", where, ref["pos0"], len(ref["run"]))
    assert tok == ref["tok"], ("id", where, ref["pos0"])
    _same(_slot_state(st, d, slot, ref["end"]), ref["snap"])


def _on(st, m=2):
    st.set_option(OPT, 1); st.set_option(MIN, m)


def _off(st):
    st.set_option(OPT, 0); st.set_option(MIN, 8)


# ---- 1: every case alone, at min = 2 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS, ids=IDS)
def test_each_run_alone_equals_the_exact_prompt_pass(model):
    st, _, d = _model(*model)
    refs = _refs(model)
    st.create_slots(len(CASES), KV_MAX)
    for s, ref in enumerate(refs):
        _fill(st, d, ref["prefix"], [s])
    assert st.multi_path_counts(reset=True)["lx"] == 0      # not vacuous: nothing was staged while the option was off, every call below is (multi_path_counts)
    _on(st)
    out = [st.extend_multi([s], [ref["run"]], [ref["pos0"]], logits=True) for s, ref in enumerate(refs)]
    took = st.multi_path_counts()
    _off(st)
    assert (took["lx"], took["lx_runs"], took["lx_short"]) == (len(CASES), len(CASES), 0), took
    for s, (ref, (ids, lg)) in enumerate(zip(refs, out)):
        _assert_run(st, d, ref, s, ids[0], lg[0], ("case", CASES[s]))


def test_short_runs_equal_decode_steps():
    """the other single-sequence reference: decode_step token by token"""
    st, _, d = _model(*MODELS[0])
    for case in (1, 3):
        ref = _refs(MODELS[0])[case]
        st.reset_decode_state(d["kv_max"])
        if ref["prefix"]:
            st.prefill(ref["prefix"], 0)
        for i, t in enumerate(ref["run"]):
            st.decode_step(t, ref["pos0"] + i)
        want = (_bits(st.read_logits()), st.last_token(), _snap(st, d, ref["end"]))
        st.create_slots(2, KV_MAX)
        _fill(st, d, ref["prefix"], [1])
        _on(st)
        ids, lg = st.extend_multi([1], [ref["run"]], [ref["pos0"]], logits=True)
        _off(st)
        assert np.array_equal(_bits(lg[0]), want[0]) and ids[0] == want[1]
        _same(_slot_state(st, d, 1, ref["end"]), want[2])


# ---- 2: a crowded call ------------------------------------------------------------------------------------------------------------------------------------------
SLOTS = [5, 0, 7, 2, 6, 11, 3, 9]                                           # slot numbers do not follow the rows


def _crowded_call(st, d, refs, on):
    """the eight runs of CASES and two unit rows in one extend_multi at min = 4 (the runs of 2 and 3 tokens stay with the run kernels), slots scrambled; slots 4 and
    10 hold state and are not in the call"""
    st.create_slots(12, KV_MAX)
    for ref, s in zip(refs, SLOTS):
        _fill(st, d, ref["prefix"], [s])
    _fill(st, d, refs[4]["prefix"], [1, 4]); _fill(st, d, refs[6]["prefix"], [8, 10])
    slots = [1] + SLOTS[:4] + [8] + SLOTS[4:]
    runs = [refs[4]["run"][:1]] + [r["run"] for r in refs[:4]] + [refs[6]["run"][:1]] + [r["run"] for r in refs[4:]]
    pos = [refs[4]["pos0"]] + [r["pos0"] for r in refs[:4]] + [refs[6]["pos0"]] + [r["pos0"] for r in refs[4:]]
    if on:
        _on(st, 4)
    ids, lg = st.extend_multi(slots, runs, pos, logits=True)
    _off(st)
    return slots, runs, pos, list(ids), lg


@pytest.mark.parametrize("model", [MODELS[0], MODELS[2], MODELS[4], MODELS[6]], ids=[IDS[0], IDS[2], IDS[4], IDS[6]])
def test_crowded_call_keeps_every_bit(model):
    st, _, d = _model(*model)
    refs = _refs(model)
    slots, runs, pos, ids0, lg0 = _crowded_call(st, d, refs, 0)
    off = [_slot_state(st, d, s, p + len(r)) for s, r, p in zip(slots, runs, pos)]
    idle = [_slot_state(st, d, 4, refs[4]["pos0"]), _slot_state(st, d, 10, refs[6]["pos0"])]
    slots, runs, pos, ids1, lg1 = _crowded_call(st, d, refs, 1)
    assert ids1 == ids0 and np.array_equal(_bits(lg1), _bits(lg0))
    for i, (s, r, p) in enumerate(zip(slots, runs, pos)):
        _same(_slot_state(st, d, s, p + len(r)), off[i])
    for row, case in zip([1, 2, 3, 4, 6, 7, 8, 9], range(8)):              # ... and each run equals the single-sequence prompt pass
        _assert_run(st, d, refs[case], slots[row], ids1[row], lg1[row], ("case", CASES[case]))
    _same(_slot_state(st, d, 4, refs[4]["pos0"]), idle[0]); _same(_slot_state(st, d, 10, refs[6]["pos0"]), idle[1])


# ---- 3: cuts ----------------------------------------------------------------------------------------------------------------------------------------------------
def _stream(st, d, prefix, run, on, cuts, paged=None):
    st.create_slots(2, KV_MAX, **(paged or {}))
    _fill(st, d, prefix, [1])
    if on:
        _on(st)
    p, i = len(prefix), 0
    for n in cuts:
        ids, lg = st.extend_multi([1], [run[i:i + n]], [p], logits=True)
        p += n; i += n
    _off(st)
    return ids[0], _bits(lg[0]), _slot_state(st, d, 1, p)


@pytest.mark.parametrize("model", [MODELS[1], MODELS[3], MODELS[5]], ids=[IDS[1], IDS[3], IDS[5]])
def test_every_cut_gives_the_bits_of_one_call(model):
    st, _, d = _model(*model)
    rng = np.random.default_rng(31)
    prefix, run = _toks(rng, d, 6), _toks(rng, d, 100)
    ref = _exact_run(st, d, prefix, run)
    for cuts in ([2, 3, 95], [17, 83], [1, 99], [100]):
        for on in (0, 1):
            tok, lg, snap = _stream(st, d, prefix, run, on, cuts)
            assert tok == ref["tok"] and np.array_equal(lg, ref["lg"]), (cuts, on)
            _same(snap, ref["snap"])


def test_prefill_slot_in_chunks():
    st, _, d = _model(*MODELS[5])
    rng = np.random.default_rng(41)
    run = _toks(rng, d, 150)
    ref = _exact_run(st, d, [], run)
    st.create_slots(2, KV_MAX)
    _on(st)
    tok = st.prefill_slot(1, run, chunk=48)                                  # 48 + 48 + 48 + 6
    _off(st)
    assert tok == ref["tok"]
    _same(_slot_state(st, d, 1, 150), ref["snap"])


# ---- 4: pages and forks -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("pt", [32, 64])
def test_paged_and_forked_slots(pt, fp8):
    model = MODELS[6] if fp8 else MODELS[5]
    st, _, d = _model(*model)
    ref = _refs(model)[7]
    st.create_slots(6, KV_MAX, page_tokens=pt, n_pages=4 * ((ref["end"] + pt - 1) // pt) + 2)
    _fill(st, d, ref["prefix"], [4, 2])
    _on(st)
    ids, lg = st.extend_multi([4], [ref["run"]], [ref["pos0"]], logits=True)
    _assert_run(st, d, ref, 4, ids[0], lg[0], "paged")
    src = _slot_state(st, d, 2, ref["pos0"])
    st.fork_slot(2, [0, 5], ref["pos0"])
    ids, lg = st.extend_multi([5, 0], [ref["run"], ref["run"]], [ref["pos0"]] * 2, logits=True)
    _off(st)
    for r, s in enumerate([5, 0]):
        _assert_run(st, d, ref, s, ids[r], lg[r], ("fork dst", s))
    _same(_slot_state(st, d, 2, ref["pos0"]), src)                          # the fork's src is untouched


# ---- 5: with the matrix-core attention of the GQA layers ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fp8", [False, True])
def test_hybrid_store_with_exact_mfma_attention(fp8):
    model = MODELS[6] if fp8 else MODELS[5]
    st, _, d = _model(*model)
    refs = _refs(model)
    st.create_slots(4, KV_MAX)
    for s, case in ((0, 7), (2, 5), (3, 1)):
        _fill(st, d, refs[case]["prefix"], [s])
    _on(st); st.set_option(XM, 1)
    ids, lg = st.extend_multi([2, 0, 3], [refs[5]["run"], refs[7]["run"], refs[1]["run"]], [refs[5]["pos0"], refs[7]["pos0"], refs[1]["pos0"]], logits=True)
    _off(st); st.set_option(XM, 0)
    for row, (s, case) in enumerate(((2, 5), (0, 7), (3, 1))):
        _assert_run(st, d, refs[case], s, ids[row], lg[row], ("xm", case))


# ---- 6: a short call after a long one ------------------------------------------------------------------------------------------------------------------------------
def test_short_call_after_a_long_one():
    """the arena rows of the first call's staged runs still hold its q / k / v / gates: the second call's rows are its own"""
    st, _, d = _model(*MODELS[0])
    refs = _refs(MODELS[0])
    st.create_slots(4, KV_MAX)
    for s, case in ((0, 7), (1, 3), (2, 1), (3, 4)):
        _fill(st, d, refs[case]["prefix"], [s])
    _on(st)
    ids, lg = st.extend_multi([0], [refs[7]["run"]], [refs[7]["pos0"]], logits=True)
    _assert_run(st, d, refs[7], 0, ids[0], lg[0], "long")
    ids, lg = st.extend_multi([3, 1, 2], [refs[4]["run"][:1], refs[3]["run"], refs[1]["run"]], [refs[4]["pos0"], refs[3]["pos0"], refs[1]["pos0"]], logits=True)
    _off(st)
    _assert_run(st, d, refs[3], 1, ids[1], lg[1], "short 5"); _assert_run(st, d, refs[1], 2, ids[2], lg[2], "short 3")
    st.create_slots(2, KV_MAX)
    _fill(st, d, refs[4]["prefix"], [1])
    unit = st.extend_multi([1], [refs[4]["run"][:1]], [refs[4]["pos0"]], logits=True)
    assert unit[0][0] == ids[0] and np.array_equal(_bits(unit[1][0]), _bits(lg[0]))


# ---- 7: the limit ---------------------------------------------------------------------------------------------------------------------------------------------------
def test_full_chunk_of_1024_tokens_from_zero_state():
    st, _, d = _model(LA, (2, 4), (128, 128), False, 1030)
    rng = np.random.default_rng(9)
    run = _toks(rng, d, 1024)
    ref = _exact_run(st, d, [], run)
    st.create_slots(2, 1030)
    _on(st)
    ids, lg = st.extend_multi([1], [run], [0], logits=True)
    _off(st)
    _assert_run(st, d, ref, 1, ids[0], lg[0], "1024 tokens")


# ---- 8: what must not change -----------------------------------------------------------------------------------------------------------------------------------------
def _other_calls(st, d, refs, on):
    """step_multi, generate_multi, verify_multi + commit_multi with a rejected draft, generate_multi_lookup"""
    pick, slots = [4, 6, 7], [3, 0, 5]
    st.create_slots(8, KV_MAX)
    for i, s in zip(pick, slots):
        _fill(st, d, refs[i]["prefix"], [s, s + 1])
    if on:
        _on(st)
    pos = [refs[i]["pos0"] for i in pick]
    firsts = [refs[i]["run"][0] for i in pick]
    out = {}
    ids, lg = st.step_multi(slots, firsts, pos, logits=True)
    out["step"] = (list(ids), _bits(lg))
    out["gen"] = st.generate_multi(slots, list(ids), [p + 1 for p in pos], 6)
    end = [p + 1 + 6 for p in pos]
    drafts = [[g[-1], (g[-1] + 1) % d["V"], 3] for g in out["gen"]]          # the model will hardly agree with these drafts
    greedy, nm = st.verify_multi(slots, drafts, end)
    keep = [min(m + 1, 2) for m in nm]
    st.commit_multi(keep)
    out["verify"] = (greedy, list(nm))
    out["states"] = [_slot_state(st, d, s, e + k) for s, e, k in zip(slots, end, keep)]
    twins = [s + 1 for s in slots]
    out["lookup"] = st.generate_multi_lookup(twins, firsts, pos, 8, contexts=[refs[i]["prefix"] + [refs[i]["run"][0]] for i in pick])
    _off(st)
    return out


def test_steps_and_verify_passes_keep_their_bits():
    st, _, d = _model(*MODELS[5])
    refs = _refs(MODELS[5])
    off, on = _other_calls(st, d, refs, 0), _other_calls(st, d, refs, 1)
    assert on["step"][0] == off["step"][0] and np.array_equal(on["step"][1], off["step"][1])
    assert on["gen"] == off["gen"] and on["verify"] == off["verify"] and on["lookup"] == off["lookup"]
    for a, b in zip(on["states"], off["states"]):
        _same(a, b)


# ---- 9: refusals, then the same call once the cause is cleared -----------------------------------------------------------------------------------------------------------
def _calls(st, V):
    t = lambda k: [x % V for x in range(1, 1 + k)]
    return (lambda: st.step_multi([1], t(1), [0]), lambda: st.extend_multi([1], [t(3)], [0]), lambda: st.generate_multi([1], t(1), [0], 2),
            lambda: st.verify_multi([1], [t(2)], [0]), lambda: st.generate_multi_lookup([1], t(1), [0], 2))


def test_the_threshold_is_checked():
    st, _, d = _model(*MODELS[0])
    for bad in (1, 0, -3, 1025):
        with pytest.raises(ValueError) as e:
            st.set_option(MIN, bad)
        assert MIN in str(e.value)
    st.set_option(MIN, 2); st.set_option(MIN, 1024); st.set_option(MIN, 8)


def test_both_long_run_options_are_refused():
    st, _, d = _model(*MODELS[0])
    ref = _refs(MODELS[0])[5]
    st.create_slots(2, KV_MAX)
    _fill(st, d, ref["prefix"], [1])
    before = _slot_state(st, d, 1, ref["pos0"])
    _on(st); st.set_option(CHUNK, 1)
    for call in list(_calls(st, d["V"])) + [lambda: st.extend_multi([1], [ref["run"]], [ref["pos0"]])]:
        _state_error(call, OPT, CHUNK)
    st.set_option(CHUNK, 0); _off(st)
    _same(_slot_state(st, d, 1, ref["pos0"]), before)                       # nothing advanced
    _on(st)
    ids, lg = st.extend_multi([1], [ref["run"]], [ref["pos0"]], logits=True)  # the cause cleared: the same call succeeds
    _off(st)
    _assert_run(st, d, ref, 1, ids[0], lg[0], "after the refusal")


def test_store_without_linear_attention_layers_is_refused():
    st, _, d = _model(("gqa", "gqa"), kv_max=32)
    st.create_slots(2, 20)
    _on(st)
    for call in _calls(st, d["V"]):
        _state_error(call, OPT, "has none")
    _off(st)
    st.step_multi([1], [1], [0])


def test_geometry_outside_the_staged_kernels_is_refused_not_run_by_the_run_kernels():
    """dv < dk: the run kernels cover it, the prompt pass's staged kernels do not"""
    st, _, d = _model(LA, (2, 4), (128, 64), False, 100)
    rng = np.random.default_rng(5)
    prefix, run = _toks(rng, d, 5), _toks(rng, d, 20)
    st.create_slots(2, 100)
    st.extend_multi([1], [prefix], [0])                                     # (the store's own prompt pass does not take this geometry either)
    before = _slot_state(st, d, 1, 5)
    _on(st)
    for call in list(_calls(st, d["V"])) + [lambda: st.extend_multi([1], [run], [5])]:
        with pytest.raises(ValueError) as e:
            call()
        assert OPT in str(e.value) and "not covered" in str(e.value), str(e.value)
    _off(st)
    _same(_slot_state(st, d, 1, 5), before)                                 # nothing ran
    ids, lg = st.extend_multi([1], [run], [5], logits=True)                 # the slot the refusals left behind takes the run kernels
    st.create_slots(2, 100)
    st.extend_multi([1], [prefix], [0])
    want = st.extend_multi([1], [run], [5], logits=True)
    assert ids[0] == want[0][0] and np.array_equal(_bits(lg[0]), _bits(want[1][0]))


def test_earlier_refusals_come_first_with_their_words():
    st, _, d = _model(*MODELS[5])
    _on(st)
    st.create_slots(2, KV_MAX)
    st.set_attention_mode(True)
    for call in _calls(st, d["V"]):
        _state_error(call, "exact-mode only")
    st.set_attention_mode(False)
    st.create_slots(2, 32, page_tokens=32, n_pages=2)                       # "multi_attn_fast" alone on paged slots is still refused with the words it had
    st.set_option("multi_attn_fast", 1)
    for call in _calls(st, d["V"]):
        _state_error(call, "does not read paged slots")
    st.set_option("multi_attn_fast", 0)
    _off(st)
