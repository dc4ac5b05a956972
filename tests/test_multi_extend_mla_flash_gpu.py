"""The "multi_extend_mla_flash" option (docs/design/27-multi-extend-mla-flash.md): a run of two or more tokens entering a device slot (extend_multi /
prefill_slot) takes the prompt pass's causal flash attention over the slot's latent and rope-key rows in its MLA layers.  Run i is BIT-IDENTICAL to
prefill(run, position) under set_attention_mode(True) on the store's own sequence holding the same prefix -- the last token's logits, the id and every latent /
rope-key row the run appends -- whatever other rows share the pass, on flat, paged and forked slots, FP16 and E4M3 caches, kv_lora_rank 512 / 256, the direct
and the LoRA query path, head counts that do and do not divide the 64-row query tile.  Runs of one token, verify passes and everything with the option off keep
their bits.  Against the exact pass the stated bound is the MLA prompt-pass flash attention's: 3e-3 with FP16 caches, 2e-2 with E4M3 caches
(docs/design/02-numerics.md 2b).

The reference is never the path under test: it is the single-sequence fast prompt pass (computed once per geometry and shared), the single-sequence fast step,
the same call with the option off, or, for the tolerance, the option-off run.  Every comparison but that one is on ids and u32 / stored-row bit patterns."""
import functools

import numpy as np
import pytest

import tests.test_multi_mla_gpu as MM
from tests.test_multi_paged_gpu import Mla, _slot_state, _state_error

pytestmark = pytest.mark.gpu
F = np.float32
U = np.uint32
OPT = "multi_extend_mla_flash"
KV_MAX = 260
# (kv_lora_rank, heads, LoRA query path, E4M3 caches): a 64-row tile cuts through a token (5, 3 heads); one token per tile (64); four tokens per tile (16)
MODELS = [(512, 5, False, False), (256, 3, False, True), (512, 64, True, True), (512, 16, False, True)]
# (tokens already in the slot, tokens of the run): one tile of two tokens; a run inside one 32-position tile; a run that starts on a tile edge; runs across
# position tiles and query-row tiles, the last one up to the last position of the store
CASES = [(0, 2), (5, 27), (32, 32), (31, 66), (37, 170), (129, 131)]
SLOTS = [5, 0, 7, 2, 6, 3]                                                  # slot numbers do not follow the rows
LONGEST = 5                                                                 # the case whose slot ends longest (260 positions)
R170 = 4                                                                    # the 170-token run

_stores = []


@pytest.fixture(autouse=True)
def options_off_afterwards():
    yield
    for st in _stores:
        st.set_option(OPT, 0); st.set_option("multi_mla_fast", 0); st.set_option("multi_extend_flash", 0); st.set_option("multi_extend_la_chunk", 0)
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


def _start(st, d, prefix):
    """the store's own sequence = prefix, by the EXACT prompt pass from zero state"""
    st.set_attention_mode(False)
    MM._start(st, d, prefix)


def _fast_run(st, d, prefix, run):
    """the single-sequence reference: the prefix by the exact prompt pass from zero state, then the run by the fast one -> logits bits, id, snapshot"""
    _start(st, d, prefix)
    st.set_attention_mode(True)
    try:
        tok = st.prefill(run, len(prefix))
        ref = dict(prefix=prefix, run=run, pos0=len(prefix), end=len(prefix) + len(run), lg=_bits(st.read_logits()), tok=tok, snap=MM._snap(st, d, len(prefix) + len(run)))
    finally:
        st.set_attention_mode(False)
    return ref


def _fast_unit(st, d, prefix, tok):
    """the single-sequence reference of a decode row: the prefix by the exact prompt pass, then decode_step under KR_ATTN_FAST"""
    _start(st, d, prefix)
    st.set_attention_mode(True)
    try:
        st.decode_step(tok, len(prefix))
        ref = dict(prefix=prefix, run=[tok], pos0=len(prefix), end=len(prefix) + 1, lg=_bits(st.read_logits()), tok=st.last_token(), snap=MM._snap(st, d, len(prefix) + 1))
    finally:
        st.set_attention_mode(False)
    return ref


@functools.lru_cache(maxsize=None)
def _refs(klr, nh, lora, fp8):
    """the six runs of CASES and their single-sequence references: computed once, shared by the tests, never modified"""
    st, _, d = _model(klr, nh, lora, fp8)
    rng = np.random.default_rng(klr + nh)
    return [_fast_run(st, d, _toks(rng, d, p), _toks(rng, d, c)) for p, c in CASES]


def _fill(st, d, prefix, slots):
    """the prefix, by the exact prompt pass on the store's own sequence, into every slot of `slots`"""
    _start(st, d, prefix)
    for s in slots:
        st.save_slot(s, len(prefix))


def _state(st, d, slot, upto):
    return _slot_state(Mla, st, d, slot, upto)


def _assert_run(st, d, ref, slot, tok, lg, where=""):
    assert np.array_equal(_bits(lg), ref["lg"]), ("logits", where, ref["pos0"], len(ref["run"]))
    assert tok == ref["tok"], ("id", where, ref["pos0"])
    MM._same(_state(st, d, slot, ref["end"]), ref["snap"])


# ---- 1: a run equals the single-sequence flash prompt pass ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("slot_seq", [260, 400])
@pytest.mark.parametrize("key", MODELS)
def test_run_equals_single_sequence_fast_prompt_pass(key, slot_seq):
    """all six runs in one call, slots scrambled: logits and id bit for bit, then every latent / rope-key row of the slot against the snapshot"""
    st, _, d = _model(*key)
    refs = _refs(*key)
    st.create_slots(8, slot_seq)
    for ref, s in zip(refs, SLOTS):
        _fill(st, d, ref["prefix"], [s])
    st.set_option(OPT, 1)
    ids, lg = st.extend_multi(SLOTS, [r["run"] for r in refs], [r["pos0"] for r in refs], logits=True)
    st.set_option(OPT, 0)
    for i, (ref, s) in enumerate(zip(refs, SLOTS)):
        _assert_run(st, d, ref, s, ids[i], lg[i], i)


# ---- 2: cut independence -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", MODELS)
def test_cuts_of_two_or_more_tokens_give_the_same_bits(key):
    """the 170-token run as 2 + 40 + 128 tokens in three calls = the run in one call (= its single-sequence reference, test 1): a 32-position tile that is fully
    masked for a row leaves the row's maximum, sum and accumulators as they were, and the positions a row sees come in the same tiles from position 0 whichever
    rows share its 64-row tile"""
    st, _, d = _model(*key)
    ref = _refs(*key)[R170]
    st.create_slots(2, KV_MAX)
    _fill(st, d, ref["prefix"], [1])
    st.set_option(OPT, 1)
    run, p0 = ref["run"], ref["pos0"]
    st.extend_multi([1], [run[:2]], [p0])
    st.extend_multi([1], [run[2:42]], [p0 + 2])
    ids, lg = st.extend_multi([1], [run[42:]], [p0 + 42], logits=True)
    st.set_option(OPT, 0)
    _assert_run(st, d, ref, 1, ids[0], lg[0], "2 + 40 + 128")


def test_prefill_slot_in_chunks_equals_the_run():
    """prefill_slot of the 170-token run in chunks of 64 tokens (64 + 64 + 42) into a slot that holds the prefix: the same bits again"""
    key = MODELS[0]
    st, _, d = _model(*key)
    ref = _refs(*key)[R170]
    st.create_slots(2, KV_MAX)
    _fill(st, d, ref["prefix"], [1])
    st.set_option(OPT, 1)
    tok = st.prefill_slot(1, ref["run"], ref["pos0"], chunk=64)
    st.set_option(OPT, 0)
    assert tok == ref["tok"]
    MM._same(_state(st, d, 1, ref["end"]), ref["snap"])


# ---- 3: unit rows beside runs --------------------------------------------------------------------------------------------------------------------------------
def _mixed(st, d, refs, rows, slot_seq, on, **slots_kw):
    """unit rows ("u": the prefix of a reference and one token) and runs ("r") in one extend_multi, rows interleaved -> (slots, ids, logits, unit slot states)"""
    st.create_slots(8, slot_seq, **slots_kw)
    slots = list(range(1, 1 + len(rows)))
    for (kind, i), s in zip(rows, slots):
        _fill(st, d, refs[i]["prefix"], [s])
    st.set_option(OPT, 1 if on else 0)
    ids, lg = st.extend_multi(slots, [refs[i]["run"][:1] if k == "u" else refs[i]["run"] for k, i in rows], [refs[i]["pos0"] for _, i in rows], logits=True)
    st.set_option(OPT, 0)
    states = [_state(st, d, s, refs[i]["pos0"] + 1) for (k, i), s in zip(rows, slots) if k == "u"]
    return slots, ids, lg, states


@pytest.mark.parametrize("key", MODELS)
def test_mixed_pass(key):
    """decode rows and prompt chunks in one pass: the unit rows carry the bits of the same call with the option off, the runs those of their references"""
    st, _, d = _model(*key)
    refs = _refs(*key)
    rows = [("u", 1), ("r", 3), ("u", 2), ("u", 5), ("r", 4)]
    _, ids0, lg0, states0 = _mixed(st, d, refs, rows, KV_MAX, False)
    slots, ids1, lg1, states1 = _mixed(st, d, refs, rows, KV_MAX, True)
    u = 0
    for r, ((kind, i), s) in enumerate(zip(rows, slots)):
        if kind == "u":
            assert np.array_equal(_bits(lg1[r]), _bits(lg0[r])) and ids1[r] == ids0[r], ("unit row", r)
            MM._same(states1[u], states0[u]); u += 1
        else:
            _assert_run(st, d, refs[i], s, ids1[r], lg1[r], ("run", r))


# ---- 4: with "multi_mla_fast" over long slots ----------------------------------------------------------------------------------------------------------------
LONG_KV = 700
LONG_KEY = MODELS[3]


@functools.lru_cache(maxsize=None)
def _long_refs():
    """above mla_split_min: a run of 130 tokens at position 520 by the fast prompt pass, unit rows at positions 650, 300 and 40 by the fast step"""
    st, _, d = _model(*LONG_KEY, kv_max=LONG_KV)
    rng = np.random.default_rng(77)
    return [_fast_run(st, d, _toks(rng, d, 520), _toks(rng, d, 130))] + [_fast_unit(st, d, _toks(rng, d, p), _toks(rng, d, 1)[0]) for p in (650, 300, 40)]


@pytest.mark.parametrize("paged", [False, True])
def test_mixed_pass_over_long_slots_with_flash_decode_rows(paged):
    """slots of 700 positions with "multi_mla_fast" also set: the unit rows take the split-KV flash-decode and carry the bits of the single-sequence fast step,
    the run those of the single-sequence fast prompt pass -- the two options compose"""
    st, _, d = _model(*LONG_KEY, kv_max=LONG_KV)
    refs = _long_refs()
    rows = [("u", 1), ("r", 0), ("u", 2), ("u", 3)]
    kw = dict(page_tokens=64, n_pages=_pages(651, 64) + _pages(650, 64) + _pages(301, 64) + _pages(41, 64) + 2) if paged else {}
    st.set_option("multi_mla_fast", 1)
    slots, ids, lg, states = _mixed(st, d, refs, rows, LONG_KV, True, **kw)
    st.set_option("multi_mla_fast", 0)
    u = 0
    for r, ((kind, i), s) in enumerate(zip(rows, slots)):
        if kind == "u":
            assert np.array_equal(_bits(lg[r]), refs[i]["lg"]) and ids[r] == refs[i]["tok"], ("unit row", r)
            MM._same(states[u], refs[i]["snap"]); u += 1
        else:
            _assert_run(st, d, refs[i], s, ids[r], lg[r], ("run", r))


# ---- 5: paged slots ------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("page_tokens", [32, 64, 256])
@pytest.mark.parametrize("key", MODELS)
def test_paged_slots_equal_flat_slots(key, page_tokens):
    """page_tokens 32: a 32-position tile is a page; 64: two tiles per page; 256: in-page offsets reach 255.  The pages of the longest run's slot are not
    consecutive: a page saved right behind its prefix's pages stays held, so the pages the run adds come from a hole below them (a spare slot saved before the
    prefix and trimmed after it) or from beyond.  Every result against the references test 1 holds the flat slots to"""
    st, _, d = _model(*key)
    refs = _refs(*key)
    pt = page_tokens
    spare, held = 1, 4
    need = sum(_pages(r["end"], pt) for r in refs)
    st.create_slots(8, KV_MAX, page_tokens=pt, n_pages=need + 3)
    for ref, s in list(zip(refs, SLOTS))[:LONGEST]:
        _fill(st, d, ref["prefix"], [s])
    st.reset_decode_state(d["kv_max"]); st.save_slot(spare, min(100, pt))      # a page between the short slots and the longest run's prefix ...
    _fill(st, d, refs[LONGEST]["prefix"], [SLOTS[LONGEST]])
    st.reset_decode_state(d["kv_max"]); st.save_slot(held, 1)               # ... and the page right behind that prefix stays held during the call
    st.trim_slot(spare, 0)                                                  # the page before it comes back as a hole: lowest free id first
    st.set_option(OPT, 1)
    ids, lg = st.extend_multi(SLOTS, [r["run"] for r in refs], [r["pos0"] for r in refs], logits=True)
    used = [int(x) for x in st.slot_page_ids(SLOTS[LONGEST])[0][:_pages(refs[LONGEST]["end"], pt)]]
    assert min(used) >= 0 and used != list(range(used[0], used[0] + len(used))), ("the longest run's pages are consecutive", used)
    st.set_option(OPT, 0)
    for i, (ref, s) in enumerate(zip(refs, SLOTS)):
        _assert_run(st, d, ref, s, ids[i], lg[i], ("paged", i))


# ---- 6: forked slots -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("page_tokens", [32, 64])
@pytest.mark.parametrize("key", [MODELS[0], MODELS[3]])
def test_run_over_a_forked_slot(key, page_tokens):
    """a slot of 129 positions forked to two destinations: position 129 is no page boundary, so the whole pages are shared and each destination gets its own
    copy of the boundary page.  The 131-token run into both destinations reads the shared pages and equals the reference; the source is unchanged"""
    st, _, d = _model(*key)
    ref = _refs(*key)[LONGEST]
    pt, src, dsts = page_tokens, 6, [4, 1]
    st.create_slots(8, KV_MAX, page_tokens=pt, n_pages=3 * _pages(ref["end"], pt))
    _fill(st, d, ref["prefix"], [src])
    st.fork_slot(src, dsts, ref["pos0"])
    full = ref["pos0"] // pt
    tables = [st.slot_page_ids(s) for s in [src] + dsts]
    for ids, refc in tables:
        assert ids[:full] == tables[0][0][:full] and refc[:full] == [3] * full      # whole pages shared by the three slots
    assert len({ids[full] for ids, _ in tables}) == 3                       # a private boundary page each
    st.set_option(OPT, 1)
    ids, lg = st.extend_multi(dsts, [ref["run"], ref["run"]], [ref["pos0"], ref["pos0"]], logits=True)
    st.set_option(OPT, 0)
    for r, s in enumerate(dsts):
        _assert_run(st, d, ref, s, ids[r], lg[r], ("fork dst", s))
        assert st.slot_page_ids(s)[0][:full] == tables[0][0][:full]         # still the shared pages
    MM._same(_state(st, d, src, ref["pos0"]), [(a[:ref["pos0"]], b[:ref["pos0"]]) for a, b in ref["snap"]])      # src untouched


# ---- 7: a pool one page short --------------------------------------------------------------------------------------------------------------------------------
def test_pool_one_page_short_fails_whole():
    key = MODELS[1]
    st, _, d = _model(*key)
    refs = _refs(*key)
    pt, pick, slots = 32, [3, 4], [2, 0]
    st.create_slots(4, KV_MAX, page_tokens=pt, n_pages=sum(_pages(refs[i]["end"], pt) for i in pick) - 1)
    for i, s in zip(pick, slots):
        _fill(st, d, refs[i]["prefix"], [s])
    before = st.slot_pages()
    states = [_state(st, d, s, refs[i]["pos0"]) for i, s in zip(pick, slots)]
    st.set_option(OPT, 1)
    _state_error(lambda: st.extend_multi(slots, [refs[i]["run"] for i in pick], [refs[i]["pos0"] for i in pick]), "does not fit the page pool")
    st.set_option(OPT, 0)
    assert st.slot_pages() == before
    for (i, s), want in zip(zip(pick, slots), states):
        MM._same(_state(st, d, s, refs[i]["pos0"]), want)


# ---- 8: nothing past the end is read -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("paged", [False, True])
@pytest.mark.parametrize("key", MODELS)
def test_rows_past_the_run_are_not_read(key, paged):
    """every row of every slot from the run's first position on holds 0xFF bytes (NaN patterns in FP16 and E4M3) before the call; the run overwrites its own
    rows, the rest -- of the last page, and of the slot's capacity -- stay.  Paged: the slots' pages were returned dirty by a slot full of such rows and handed
    out again.  Finite, and equal to the references"""
    st, _, d = _model(*key)
    refs = _refs(*key)
    esz = np.uint8 if d["fp8"] else np.uint16
    kw = dict(page_tokens=32, n_pages=6 * _pages(KV_MAX, 32)) if paged else {}
    st.create_slots(8, KV_MAX, **kw)

    def poisoned(prefix, slot):
        """the slot holds the prefix's rows and 0xFF in every row behind them, up to the slot's end"""
        _start(st, d, prefix)
        rows = []
        for li in range(d["nL"]):
            ck = np.empty((d["kv_max"], d["klr"]), esz); kp = np.empty((d["kv_max"], d["rd"]), esz)
            st.get_decode_state(li, ck, kp, None, None)
            ck[len(prefix):] = np.iinfo(esz).max; kp[len(prefix):] = np.iinfo(esz).max
            rows.append((ck, kp))
        z = [0] * d["nL"]
        st.set_decode_state(len(prefix), d["kv_max"], z, z, z, z, [a.ctypes.data for a, _ in rows], [b.ctypes.data for _, b in rows])
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


# ---- 9: a full chunk -----------------------------------------------------------------------------------------------------------------------------------------
def test_full_chunk_of_1024_tokens():
    """one run of KR_EXTEND_MAX_TOKENS tokens at position 60 into a slot of 1100 positions (kv_lora_rank 256, 3 heads, E4M3: 48 query-row tiles).  The store's
    fast prompt pass takes 1024 tokens as one chunk by default: its result is that of a pass told to use chunks of 1024"""
    key = MODELS[1]
    st, _, d = _model(*key, kv_max=1100)
    rng = np.random.default_rng(9)
    prefix, run = _toks(rng, d, 60), _toks(rng, d, 1024)
    ref = _fast_run(st, d, prefix, run)
    st.set_prefill_chunk(1024)
    one = _fast_run(st, d, prefix, run)
    st.set_prefill_chunk(0)
    assert np.array_equal(one["lg"], ref["lg"]) and one["tok"] == ref["tok"]
    MM._same(one["snap"], ref["snap"])
    st.create_slots(2, 1100)
    _fill(st, d, prefix, [1])
    st.set_option(OPT, 1)
    ids, lg = st.extend_multi([1], [run], [60], logits=True)
    st.set_option(OPT, 0)
    _assert_run(st, d, ref, 1, ids[0], lg[0], "1024 tokens")


# ---- 10: the stated tolerance against the exact pass ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", MODELS)
def test_within_the_prompt_flash_bound_of_the_exact_pass(key):
    """the 170-token run with the option off and on: max |on - off| <= 3e-3 max |off| with FP16 caches, 2e-2 with E4M3 caches (docs/design/02-numerics.md 2b,
    tests/test_attn_fast_gpu.py) on the run's last-token logits and on the next step_multi on the state left behind; the greedy id is the same with FP16 caches.
    The bits differ somewhere: the option is no silent fall-back to the exact kernels"""
    st, _, d = _model(*key)
    ref = _refs(*key)[R170]
    bound = 2e-2 if d["fp8"] else 3e-3
    out = []
    for on in (0, 1):
        st.create_slots(2, KV_MAX)
        _fill(st, d, ref["prefix"], [1])
        st.set_option(OPT, on)
        ids, lg = st.extend_multi([1], [ref["run"]], [ref["pos0"]], logits=True)
        ids2, lg2 = st.step_multi([1], [ids[0]], [ref["end"]], logits=True)
        st.set_option(OPT, 0)
        out.append((ids[0], lg[0].copy(), ids2[0], lg2[0].copy()))
    (t0, l0, n0, m0), (t1, l1, n1, m1) = out
    r_run = float(np.abs(l1 - l0).max() / np.abs(l0).max()); r_next = float(np.abs(m1 - m0).max() / np.abs(m0).max())
    print("multi_extend_mla_flash %s %s: run %.3e  next step %.3e (bound %.0e)" % (key, "E4M3" if d["fp8"] else "FP16", r_run, r_next, bound))
    assert r_run <= bound and r_next <= bound, (r_run, r_next)
    if not d["fp8"]:
        assert t1 == t0
    assert not np.array_equal(_bits(l1), _bits(l0))                         # the run kernel ran


# ---- 11: what must not change --------------------------------------------------------------------------------------------------------------------------------
def _unchanged_calls(st, d, refs, on):
    """unit runs by extend_multi, step_multi, generate_multi, verify_multi + commit_multi with a rejected draft, generate_multi_lookup: everything they return
    and leave behind"""
    pick, slots = [1, 2, 3], [3, 0, 5]
    st.create_slots(8, KV_MAX)
    for i, s in zip(pick, slots):
        _fill(st, d, refs[i]["prefix"], [s, s + 1])
    st.set_option(OPT, on)
    pos = [refs[i]["pos0"] for i in pick]
    firsts = [refs[i]["run"][0] for i in pick]
    out = {}
    ids, lg = st.extend_multi(slots, [[f] for f in firsts], pos, logits=True)      # runs of one token
    out["unit"] = (list(ids), _bits(lg))
    ids, lg = st.step_multi(slots, firsts, pos, logits=True)                # the same rows again: rows at pos are overwritten
    out["step"] = (list(ids), _bits(lg))
    out["gen"] = st.generate_multi(slots, list(ids), [p + 1 for p in pos], 6)
    end = [p + 1 + 6 for p in pos]
    drafts = [[g[-1], (g[-1] + 1) % d["V"], 3] for g in out["gen"]]          # the model will hardly agree with these drafts
    greedy, nm = st.verify_multi(slots, drafts, end)
    keep = [min(m + 1, 2) for m in nm]
    st.commit_multi(keep)
    out["verify"] = (greedy, list(nm))
    out["states"] = [_state(st, d, s, e + k) for s, e, k in zip(slots, end, keep)]
    twins = [s + 1 for s in slots]
    out["plain"] = st.generate_multi(twins, firsts, pos, 8)
    for i, s in zip(pick, twins):
        _fill(st, d, refs[i]["prefix"], [s])
    out["lookup"] = st.generate_multi_lookup(twins, firsts, pos, 8, contexts=[refs[i]["prefix"] + [refs[i]["run"][0]] for i in pick])
    st.set_option(OPT, 0)
    return out


def test_unit_runs_and_verify_passes_keep_their_bits():
    key = MODELS[0]
    st, _, d = _model(*key)
    refs = _refs(*key)
    off, on = _unchanged_calls(st, d, refs, 0), _unchanged_calls(st, d, refs, 1)
    for k in ("unit", "step"):
        assert on[k][0] == off[k][0] and np.array_equal(on[k][1], off[k][1]), k
    assert on["unit"][0] == on["step"][0] and np.array_equal(on["unit"][1], on["step"][1])
    assert on["gen"] == off["gen"] and on["verify"] == off["verify"] and on["plain"] == off["plain"]
    for a, b in zip(on["states"], off["states"]):
        MM._same(a, b)
    assert on["lookup"] == on["plain"]                                      # speculation stays exact under the option


# ---- 12: refusals, then option 0 -----------------------------------------------------------------------------------------------------------------------------
def _calls(st, V):
    t = lambda k: [x % V for x in range(1, 1 + k)]
    return (lambda: st.step_multi([1], t(1), [0]), lambda: st.extend_multi([1], [t(3)], [0]), lambda: st.prefill_slot(1, t(5), 0), lambda: st.generate_multi([1], t(1), [0], 2),
            lambda: st.verify_multi([1], [t(2)], [0]), lambda: st.generate_multi_lookup([1], t(1), [0], 2))


def test_store_without_mla_layers_is_refused():
    from tests.test_decode_gpu import build
    st, eng, orc, keep, d = build(seed=3, kv_max=32)                        # linear attention + GQA
    _stores.append(st)
    st.create_slots(2, 20)
    want = st.extend_multi([1], [[1, 2, 3]], [0], logits=True)
    st.set_option(OPT, 1)
    for call in _calls(st, d["V"]):
        _state_error(call, OPT, "has none")
    st.set_option(OPT, 0)
    st.create_slots(2, 20)
    got = st.extend_multi([1], [[1, 2, 3]], [0], logits=True)
    assert got[0] == want[0] and np.array_equal(_bits(got[1]), _bits(want[1]))


def test_other_refusals_stay_and_option_zero_is_the_exact_pass():
    key = MODELS[0]
    st, _, d = _model(*key)
    ref = _refs(*key)[3]

    def run():
        st.create_slots(2, KV_MAX)
        _fill(st, d, ref["prefix"], [1])
        ids, lg = st.extend_multi([1], [ref["run"]], [ref["pos0"]], logits=True)
        return ids[0], _bits(lg[0]), _state(st, d, 1, ref["end"])

    exact = run()
    st.set_option(OPT, 1)
    st.create_slots(2, KV_MAX)
    st.set_attention_mode(True)                                             # the mode bits stay refused
    for call in _calls(st, d["V"]):
        _state_error(call, "exact-mode only")
    st.set_attention_mode(False)
    st.set_option("multi_extend_flash", 1)                                  # the GQA run option keeps its refusal of a store with an MLA layer, and its words
    for call in _calls(st, d["V"]):
        _state_error(call, '"multi_extend_flash" option covers GQA layers only', "is MLA")
    st.set_option("multi_extend_flash", 0)
    st.set_option("multi_extend_la_chunk", 1)                               # so does the linear-attention one
    for call in _calls(st, d["V"]):
        _state_error(call, '"multi_extend_la_chunk" option covers linear-attention layers only')
    st.set_option("multi_extend_la_chunk", 0)
    st.create_slots(2, KV_MAX, page_tokens=32, n_pages=4)                   # "multi_attn_fast" on an MLA store is refused first, with the words it had
    st.set_option("multi_attn_fast", 1)
    for call in _calls(st, d["V"]):
        _state_error(call, '"multi_attn_fast" option covers GQA layers only')
    st.set_option("multi_attn_fast", 0)
    st.set_option(OPT, 0)
    again = run()
    assert again[0] == exact[0] and np.array_equal(again[1], exact[1])
    MM._same(again[2], exact[2])
