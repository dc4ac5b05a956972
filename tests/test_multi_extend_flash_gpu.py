"""The "multi_extend_flash" option (docs/design/25-multi-extend-flash.md): a run of two or more tokens entering a device slot (extend_multi / prefill_slot) takes
the prompt pass's causal flash attention over the slot in its GQA layers.  On a store whose attention layers are all GQA, run i is BIT-IDENTICAL to
prefill(run, position) under set_attention_mode(True) on a store whose own sequence holds the same prefix -- the last token's logits, the id and every K / V row
the run appends -- whatever other rows share the pass, on flat and paged slots, FP16 and E4M3, head_dim 64 / 128 / 256.  Runs of one token, verify passes and
everything with the option off keep their bits.  On a hybrid store (linear attention + GQA) the linear-attention runs stay exact and the stated bound is the
prompt-pass flash attention's 3e-3 (docs/design/02-numerics.md 2b).

The reference is never the path under test: it is the single-sequence fast prompt pass (computed once per geometry and shared), the same call with the option
off, or, for the tolerance, the option-off run.  Every comparison but that one is on ids and u32 / stored-row bit patterns."""
import functools

import numpy as np
import pytest

from tests.test_decode_gpu import build
from tests.test_multi_paged_gpu import _state_error
from tests.test_speculative_gpu import _same, _snap

pytestmark = pytest.mark.gpu
F = np.float32
U = np.uint32
OPT = "multi_extend_flash"
KV_MAX = 260
# (head_dim, query heads on 2 KV heads, E4M3): both kernel forms (head_dim >= 128: wave-specialised) and query tiles of 16, 32, 64 and 16 tokens
MODELS = [(256, 16, False), (128, 8, True), (64, 4, False), (64, 16, True)]
# (tokens already in the slot, tokens of the run): one tile of two rows; a run inside one 64-position tile; a run that starts on a tile edge and fills a 64-token
# query tile; runs across the query-tile (16 / 32 / 64 tokens), 64-position-tile and 32-row-block edges, the last one up to the last position of the store
CASES = [(0, 2), (5, 63), (64, 64), (63, 130), (37, 170), (129, 131)]
SLOTS = [5, 0, 7, 2, 6, 3]                                                  # slot numbers do not follow the rows
LONGEST = 5                                                                 # the case whose slot ends longest (260 positions)

_stores = []


@pytest.fixture(autouse=True)
def options_off_afterwards():
    yield
    for st in _stores:
        st.set_option(OPT, 0); st.set_option("multi_attn_fast", 0); st.set_option("multi_attn_fast_paged", 0); st.set_attention_mode(False)


def _toks(rng, d, n):
    return [int(x) for x in rng.integers(0, d["V"], n)]


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
    _stores.append(st)
    return st, (eng, orc, keep), d


def _fast_run(st, d, prefix, run):
    """the single-sequence reference: the prefix by the exact prompt pass from zero state, then the run by the fast one -> logits bits, id, snapshot"""
    st.set_attention_mode(False)
    st.reset_decode_state(d["kv_max"])
    if prefix:
        st.prefill(prefix, 0)
    st.set_attention_mode(True)
    tok = st.prefill(run, len(prefix))
    ref = dict(prefix=prefix, run=run, pos0=len(prefix), end=len(prefix) + len(run), lg=_bits(st.read_logits()), tok=tok, snap=_snap(st, d, len(prefix) + len(run)))
    st.set_attention_mode(False)
    return ref


@functools.lru_cache(maxsize=None)
def _refs(hd, nh, fp8):
    """the six runs of CASES and their single-sequence references: computed once, shared by the tests, never modified"""
    st, _, d = _model(hd, nh, fp8)
    rng = np.random.default_rng(hd + nh)
    return [_fast_run(st, d, _toks(rng, d, p), _toks(rng, d, c)) for p, c in CASES]


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


# ---- 1: a run equals the single-sequence flash prompt pass ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("slot_seq", [260, 400])
@pytest.mark.parametrize("hd,nh,fp8", MODELS)
def test_run_equals_single_sequence_fast_prompt_pass(hd, nh, fp8, slot_seq):
    """all six runs in one call, slots scrambled: logits and id bit for bit, then every K / V row of the slot against the snapshot"""
    st, _, d = _model(hd, nh, fp8)
    refs = _refs(hd, nh, fp8)
    st.create_slots(8, slot_seq)
    for ref, s in zip(refs, SLOTS):
        _fill(st, d, ref["prefix"], [s])
    st.set_option(OPT, 1)
    ids, lg = st.extend_multi(SLOTS, [r["run"] for r in refs], [r["pos0"] for r in refs], logits=True)
    st.set_option(OPT, 0)
    for i, (ref, s) in enumerate(zip(refs, SLOTS)):
        _assert_run(st, d, ref, s, ids[i], lg[i], i)


# ---- 2: cut independence -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hd,nh,fp8", MODELS)
def test_cuts_of_two_or_more_tokens_give_the_same_bits(hd, nh, fp8):
    """the 170-token run as 2 + 40 + 128 tokens in three calls = the run in one call (= its single-sequence reference, test 1): a tile that is fully masked for a
    row leaves the row's maximum, sum and accumulators as they were, in both kernel forms"""
    st, _, d = _model(hd, nh, fp8)
    ref = _refs(hd, nh, fp8)[4]
    st.create_slots(2, KV_MAX)
    _fill(st, d, ref["prefix"], [1])
    st.set_option(OPT, 1)
    run, p0 = ref["run"], ref["pos0"]
    st.extend_multi([1], [run[:2]], [p0])
    st.extend_multi([1], [run[2:42]], [p0 + 2])
    ids, lg = st.extend_multi([1], [run[42:]], [p0 + 42], logits=True)
    st.set_option(OPT, 0)
    _assert_run(st, d, ref, 1, ids[0], lg[0], "2 + 40 + 128")


# ---- 3: unit rows beside runs --------------------------------------------------------------------------------------------------------------------------------
def _mixed(st, d, refs, units, longs, slot_seq, on, **slots_kw):
    """three unit rows (the prefixes of `units`, one token each) and the runs of `longs` in one extend_multi, rows interleaved -> (ids, logits, unit slot states)"""
    rows = [("u", units[0]), ("r", longs[0]), ("u", units[1]), ("u", units[2]), ("r", longs[1])] if len(longs) == 2 else [("u", units[0]), ("r", longs[0]), ("u", units[1]), ("u", units[2])]
    st.create_slots(8, slot_seq, **slots_kw)
    slots = list(range(1, 1 + len(rows)))
    for (kind, i), s in zip(rows, slots):
        _fill(st, d, refs[i]["prefix"], [s])
    st.set_option(OPT, 1 if on else 0)
    ids, lg = st.extend_multi(slots, [refs[i]["run"][:1] if k == "u" else refs[i]["run"] for k, i in rows], [refs[i]["pos0"] for _, i in rows], logits=True)
    st.set_option(OPT, 0)
    states = [_slot_state(st, d, s, refs[i]["pos0"] + 1) for (k, i), s in zip(rows, slots) if k == "u"]
    return rows, slots, ids, lg, states


@pytest.mark.parametrize("hd,nh,fp8", MODELS)
def test_mixed_pass(hd, nh, fp8):
    """decode rows and prompt chunks in one pass: the unit rows carry the bits of the same call with the option off, the runs those of their references"""
    st, _, d = _model(hd, nh, fp8)
    refs = _refs(hd, nh, fp8)
    units, longs = [1, 2, 5], [3, 4]
    _, _, ids0, lg0, states0 = _mixed(st, d, refs, units, longs, KV_MAX, False)
    rows, slots, ids1, lg1, states1 = _mixed(st, d, refs, units, longs, KV_MAX, True)
    u = 0
    for r, ((kind, i), s) in enumerate(zip(rows, slots)):
        if kind == "u":
            assert np.array_equal(_bits(lg1[r]), _bits(lg0[r])) and ids1[r] == ids0[r], ("unit row", r)
            _same(states1[u], states0[u]); u += 1
        else:
            _assert_run(st, d, refs[i], s, ids1[r], lg1[r], ("run", r))


LONG_KV = 1300


@functools.lru_cache(maxsize=None)
def _long_refs():
    """above gqa_split_min: unit rows at positions 1100, 700 and 40 and a run of 130 tokens at position 1100 (head_dim 128, E4M3: the wave-specialised form)"""
    st, _, d = _model(128, 8, True, kv_max=LONG_KV)
    rng = np.random.default_rng(77)
    return [_fast_run(st, d, _toks(rng, d, p), _toks(rng, d, c)) for p, c in [(1100, 130), (700, 2), (40, 2), (1100, 2)]]


@pytest.mark.parametrize("paged", [False, True])
def test_mixed_pass_over_long_slots_with_flash_decode_rows(paged):
    """slots of 1300 positions with "multi_attn_fast_paged" also set: the unit rows take the split-KV flash-decode and equal the call under that option alone; the
    run equals its single-sequence reference"""
    st, _, d = _model(128, 8, True, kv_max=LONG_KV)
    refs = _long_refs()
    kw = dict(page_tokens=64, n_pages=3 * _pages(1101, 64) + _pages(1230, 64) + _pages(701, 64) + _pages(41, 64) + 2) if paged else {}
    st.set_option("multi_attn_fast_paged", 1)
    _, _, ids0, lg0, states0 = _mixed(st, d, refs, [3, 1, 2], [0], LONG_KV, False, **kw)
    rows, slots, ids1, lg1, states1 = _mixed(st, d, refs, [3, 1, 2], [0], LONG_KV, True, **kw)
    st.set_option("multi_attn_fast_paged", 0)
    u = 0
    for r, ((kind, i), s) in enumerate(zip(rows, slots)):
        if kind == "u":
            assert np.array_equal(_bits(lg1[r]), _bits(lg0[r])) and ids1[r] == ids0[r], ("unit row", r)
            _same(states1[u], states0[u]); u += 1
        else:
            _assert_run(st, d, refs[i], s, ids1[r], lg1[r], ("run", r))


# ---- 4: paged slots ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("page_tokens", [32, 64, 256])
@pytest.mark.parametrize("hd,nh,fp8", MODELS)
def test_paged_slots_equal_flat_slots(hd, nh, fp8, page_tokens):
    """page_tokens 32: a 64-position tile spans two pages; 64: a tile is a page; 256: in-page offsets reach 255.  The pages of the longest run's slot are not
    consecutive: a page saved right behind its prefix's pages stays held, so the pages the run adds come from a hole below them (a spare slot saved before the
    prefix and trimmed after it) or from beyond.  Then a fork at position 129 (whole pages shared, the boundary page copied) and the run into both dsts.  Every
    result against the references test 1 holds the flat slots to"""
    st, _, d = _model(hd, nh, fp8)
    refs = _refs(hd, nh, fp8)
    pt = page_tokens
    spare, dsts = 1, [4, 1]
    need = sum(_pages(r["end"], pt) for r in refs) + 2 * _pages(refs[LONGEST]["end"], pt)
    st.create_slots(8, KV_MAX, page_tokens=pt, n_pages=need + 2)
    for ref, s in list(zip(refs, SLOTS))[:LONGEST]:
        _fill(st, d, ref["prefix"], [s])
    st.reset_decode_state(d["kv_max"]); st.save_slot(spare, min(100, pt))      # a page between the short slots and the longest run's prefix ...
    _fill(st, d, refs[LONGEST]["prefix"], [SLOTS[LONGEST]])
    st.reset_decode_state(d["kv_max"]); st.save_slot(dsts[0], 1)            # ... and the page right behind that prefix stays held during the call
    st.trim_slot(spare, 0)                                                  # the page before it comes back as a hole: lowest free id first
    st.set_option(OPT, 1)
    ids, lg = st.extend_multi(SLOTS, [r["run"] for r in refs], [r["pos0"] for r in refs], logits=True)
    used = [int(x) for x in st.slot_page_ids(SLOTS[LONGEST])[0][:_pages(refs[LONGEST]["end"], pt)]]
    assert min(used) >= 0 and used != list(range(used[0], used[0] + len(used))), ("the longest run's pages are consecutive", used)
    st.set_option(OPT, 0)
    for i, (ref, s) in enumerate(zip(refs, SLOTS)):
        _assert_run(st, d, ref, s, ids[i], lg[i], ("paged", i))
    # fork: the prefix of the longest case again, shared by two dsts
    ref = refs[LONGEST]
    for s in SLOTS[:LONGEST]:
        st.trim_slot(s, 0)
    st.trim_slot(SLOTS[LONGEST], ref["pos0"])
    st.fork_slot(SLOTS[LONGEST], dsts, ref["pos0"])
    if ref["pos0"] >= pt:
        assert st.slot_page_ids(dsts[0])[0][0] == st.slot_page_ids(SLOTS[LONGEST])[0][0] and st.slot_page_ids(dsts[0])[1][0] == 3      # page 0: one copy, three holders
    st.set_option(OPT, 1)
    ids, lg = st.extend_multi(dsts, [ref["run"], ref["run"]], [ref["pos0"], ref["pos0"]], logits=True)
    st.set_option(OPT, 0)
    for r, s in enumerate(dsts):
        _assert_run(st, d, ref, s, ids[r], lg[r], ("fork dst", s))
    _same(_slot_state(st, d, SLOTS[LONGEST], ref["pos0"]), [(k, li, a[:ref["pos0"]], b[:ref["pos0"]]) for k, li, a, b in ref["snap"]])      # src untouched


@pytest.mark.parametrize("hd,nh,fp8", [(128, 8, True)])
def test_pool_one_page_short_fails_whole(hd, nh, fp8):
    st, _, d = _model(hd, nh, fp8)
    refs = _refs(hd, nh, fp8)
    pt, pick = 32, [3, 4]
    st.create_slots(4, KV_MAX, page_tokens=pt, n_pages=sum(_pages(refs[i]["end"], pt) for i in pick) - 1)
    for i, s in zip(pick, [2, 0]):
        _fill(st, d, refs[i]["prefix"], [s])
    before = st.slot_pages()
    states = [_slot_state(st, d, s, refs[i]["pos0"]) for i, s in zip(pick, [2, 0])]
    st.set_option(OPT, 1)
    _state_error(lambda: st.extend_multi([2, 0], [refs[i]["run"] for i in pick], [refs[i]["pos0"] for i in pick]), "does not fit the page pool")
    st.set_option(OPT, 0)
    assert st.slot_pages() == before
    for (i, s), want in zip(zip(pick, [2, 0]), states):
        _same(_slot_state(st, d, s, refs[i]["pos0"]), want)


# ---- 5: nothing past the end is read -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("paged", [False, True])
@pytest.mark.parametrize("hd,nh,fp8", MODELS)
def test_rows_past_the_run_are_not_read(hd, nh, fp8, paged):
    """every row of every slot from the run's first position on holds 0xFF bytes (NaN patterns in FP16 and E4M3) before the call; the run overwrites its own
    rows, the rest stay.  Paged: the slots' pages were returned dirty by a slot full of such rows and handed out again.  Finite, and equal to the references"""
    st, _, d = _model(hd, nh, fp8)
    refs = _refs(hd, nh, fp8)
    esz = np.uint8 if fp8 else np.uint16
    width = d["nkv"] * d["hd"]
    kw = dict(page_tokens=32, n_pages=6 * _pages(KV_MAX, 32)) if paged else {}
    st.create_slots(8, KV_MAX, **kw)

    def poisoned(prefix, slot):
        """the slot holds the prefix's rows and 0xFF in every row behind them, up to the slot's end"""
        st.reset_decode_state(d["kv_max"])
        if prefix:
            st.prefill(prefix, 0)
        rows = []
        for li in range(len(d["kinds"])):
            kc = np.empty((d["kv_max"], width), esz); vc = np.empty_like(kc)
            st.get_decode_state(li, kc, vc, None, None)
            kc[len(prefix):] = np.iinfo(esz).max; vc[len(prefix):] = np.iinfo(esz).max
            rows.append((kc, vc))
        st.set_decode_state(len(prefix), d["kv_max"], [k.ctypes.data for k, _ in rows], [v.ctypes.data for _, v in rows], [0] * len(rows), [0] * len(rows))
        st.save_slot(slot, KV_MAX)

    if paged:
        for s in SLOTS:
            poisoned([], s)
        for s in SLOTS:
            st.trim_slot(s, 0)                                              # every page of the pool goes back dirty
    for ref, s in zip(refs, SLOTS):
        poisoned(ref["prefix"], s)
    st.set_option(OPT, 1)
    ids, lg = st.extend_multi(SLOTS, [r["run"] for r in refs], [r["pos0"] for r in refs], logits=True)
    st.set_option(OPT, 0)
    assert np.isfinite(lg).all()
    for i, (ref, s) in enumerate(zip(refs, SLOTS)):
        _assert_run(st, d, ref, s, ids[i], lg[i], ("poisoned", i))


# ---- 6: a full chunk -----------------------------------------------------------------------------------------------------------------------------------------
def test_full_chunk_of_1024_tokens():
    """one run of KR_EXTEND_MAX_TOKENS tokens at position 100 into a slot of 1200 positions.  The store's fast prompt pass takes 1024 tokens as one chunk by
    default: its result is that of a pass told to use chunks of 1024"""
    st, _, d = _model(64, 4, False, kv_max=1200)
    rng = np.random.default_rng(9)
    prefix, run = _toks(rng, d, 100), _toks(rng, d, 1024)
    ref = _fast_run(st, d, prefix, run)
    st.set_prefill_chunk(1024)
    one = _fast_run(st, d, prefix, run)
    st.set_prefill_chunk(0)
    assert np.array_equal(one["lg"], ref["lg"]) and one["tok"] == ref["tok"]
    _same(one["snap"], ref["snap"])
    st.create_slots(2, 1200)
    _fill(st, d, prefix, [1])
    st.set_option(OPT, 1)
    ids, lg = st.extend_multi([1], [run], [100], logits=True)
    st.set_option(OPT, 0)
    _assert_run(st, d, ref, 1, ids[0], lg[0], "1024 tokens")


# ---- 7: hybrid stores, the stated tolerance ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fp8", [False, True])
def test_hybrid_store_within_the_prompt_flash_bound(fp8):
    """linear attention + GQA (the default test model): the linear-attention runs stay exact, so there is no single-sequence equal; the bound is the prompt-pass
    flash attention's, max |on - off| <= 3e-3 max |off| (docs/design/02-numerics.md 2b) on the run's last-token logits and on the next step_multi on the state
    left behind; the greedy id is the same"""
    st, _, d = _model(64, 4, fp8, kinds=("la", "gqa", "la"))
    rng = np.random.default_rng(21)
    prefix, run = _toks(rng, d, 37), _toks(rng, d, 170)
    out = []
    for on in (0, 1):
        st.create_slots(2, KV_MAX)
        _fill(st, d, prefix, [1])
        st.set_option(OPT, on)
        ids, lg = st.extend_multi([1], [run], [37], logits=True)
        ids2, lg2 = st.step_multi([1], [ids[0]], [37 + 170], logits=True)
        st.set_option(OPT, 0)
        out.append((ids[0], lg[0].copy(), ids2[0], lg2[0].copy()))
    (t0, l0, n0, m0), (t1, l1, n1, m1) = out
    r_run = float(np.abs(l1 - l0).max() / np.abs(l0).max()); r_next = float(np.abs(m1 - m0).max() / np.abs(m0).max())
    print("multi_extend_flash hybrid %s: run %.3e  next step %.3e (bound 3e-3)" % ("E4M3" if fp8 else "FP16", r_run, r_next))
    assert r_run <= 3e-3 and r_next <= 3e-3, (r_run, r_next)
    assert t1 == t0 and n1 == n0


# ---- 8: what must not change ---------------------------------------------------------------------------------------------------------------------------------
def _unchanged_calls(st, d, refs, on):
    """step_multi, generate_multi, verify_multi + commit_multi with a rejected draft, generate_multi_lookup: everything they return and leave behind"""
    pick, slots = [1, 2, 3], [3, 0, 5]
    st.create_slots(8, KV_MAX)
    for i, s in zip(pick, slots):
        _fill(st, d, refs[i]["prefix"], [s, s + 1])
    st.set_option(OPT, on)
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
    out["plain"] = st.generate_multi(twins, firsts, pos, 8)
    for i, s in zip(pick, twins):
        _fill(st, d, refs[i]["prefix"], [s])
    out["lookup"] = st.generate_multi_lookup(twins, firsts, pos, 8, contexts=[refs[i]["prefix"] + [refs[i]["run"][0]] for i in pick])
    st.set_option(OPT, 0)
    return out


def test_unit_runs_and_verify_passes_keep_their_bits():
    st, _, d = _model(64, 4, False)
    refs = _refs(64, 4, False)
    off, on = _unchanged_calls(st, d, refs, 0), _unchanged_calls(st, d, refs, 1)
    assert on["step"][0] == off["step"][0] and np.array_equal(on["step"][1], off["step"][1])
    assert on["gen"] == off["gen"] and on["verify"] == off["verify"] and on["plain"] == off["plain"]
    for a, b in zip(on["states"], off["states"]):
        _same(a, b)
    assert on["lookup"] == on["plain"]                                      # speculation stays exact under the option


# ---- 9: refusals, then option 0 ------------------------------------------------------------------------------------------------------------------------------
def _calls(st, V):
    t = lambda k: [x % V for x in range(1, 1 + k)]
    return (lambda: st.step_multi([1], t(1), [0]), lambda: st.extend_multi([1], [t(3)], [0]), lambda: st.generate_multi([1], t(1), [0], 2),
            lambda: st.verify_multi([1], [t(2)], [0]), lambda: st.generate_multi_lookup([1], t(1), [0], 2))


def test_mla_store_is_refused():
    from tests.test_mla_gpu import build as build_mla
    st, eng, orc, keep, d = build_mla(kv_max=24)
    _stores.append(st)
    st.create_slots(2, 20)
    st.set_option(OPT, 1)
    for call in _calls(st, d["V"]):
        _state_error(call, OPT, "MLA")
    st.set_option(OPT, 0)
    st.step_multi([1], [1], [0])


def test_store_without_gqa_layers_is_refused():
    st, _, d = _model(64, 4, False, kv_max=32, kinds=("la", "la"))
    st.create_slots(2, 20)
    st.set_option(OPT, 1)
    for call in _calls(st, d["V"]):
        _state_error(call, OPT, "has none")
    st.set_option(OPT, 0)
    st.step_multi([1], [1], [0])


def test_group_of_six_heads_is_refused_not_run_exactly():
    st, _, d = _model(64, 12, False, kv_max=32)
    st.create_slots(2, 20)
    want = st.extend_multi([1], [[1, 2, 3]], [0], logits=True)
    st.set_option(OPT, 1)
    for call in _calls(st, d["V"]):
        with pytest.raises(ValueError) as e:
            call()
        assert OPT in str(e.value) and "divide 128" in str(e.value), str(e.value)
    # "multi_attn_fast" alone on paged slots is still refused first, with the words it had
    st.create_slots(2, 32, page_tokens=32, n_pages=2)
    st.set_option("multi_attn_fast", 1)
    for call in _calls(st, d["V"]):
        _state_error(call, "does not read paged slots")
    st.set_option("multi_attn_fast", 0)
    st.set_option(OPT, 0)
    st.create_slots(2, 20)
    got = st.extend_multi([1], [[1, 2, 3]], [0], logits=True)
    assert got[0] == want[0] and np.array_equal(_bits(got[1]), _bits(want[1]))


def test_mode_bits_stay_refused_and_option_zero_is_the_exact_pass():
    st, _, d = _model(64, 4, False)
    ref = _refs(64, 4, False)[3]

    def run():
        st.create_slots(2, KV_MAX)
        _fill(st, d, ref["prefix"], [1])
        ids, lg = st.extend_multi([1], [ref["run"]], [ref["pos0"]], logits=True)
        return ids[0], _bits(lg[0]), _slot_state(st, d, 1, ref["end"])

    exact = run()
    st.set_option(OPT, 1)
    st.create_slots(2, KV_MAX)
    st.set_attention_mode(True)
    for call in _calls(st, d["V"]):
        _state_error(call, "exact-mode only")
    st.set_attention_mode(False)
    st.set_option(OPT, 0)
    again = run()
    assert again[0] == exact[0] and np.array_equal(again[1], exact[1])
    _same(again[2], exact[2])
