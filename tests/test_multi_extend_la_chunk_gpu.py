"""The "multi_extend_la_chunk" option (docs/design/26-multi-extend-la-chunk.md): a run of 64 or more tokens entering a device slot (extend_multi / prefill_slot)
takes the prompt pass's chunked delta rule in its linear-attention layers.  On a store whose attention layers are all linear attention, and on a hybrid store
(linear attention + GQA) with "multi_extend_flash" set as well, run i is BIT-IDENTICAL to prefill(run, position) under set_attention_mode(True) on a store whose
own sequence holds the same prefix -- the last token's logits, the id, the conv and recurrent state left in the slot and every K / V row the run appends --
whatever other rows share the pass, on flat and paged slots.  Shorter runs, verify passes and everything with the option off keep their bits.

The reference is never the path under test: it is the single-sequence fast prompt pass (computed once per model and shared), the same call with the option off,
or, for the tolerances, the option-off run.  Every comparison but those is on ids and u32 / stored-row bit patterns.

Observed on an MI355X, 37 tokens in the slot and a run of 170 (max |on - off| / max |off|: the run's last-token logits, the next step_multi): la + la 1.4e-4,
1.8e-4 (bound 1e-3); la + gqa + la under this option alone FP16 2.5e-4, 1.5e-4, E4M3 3.0e-4, 1.8e-4 (bound 3e-3).  192 tokens as 100 + 92 against the exact run:
1.2e-4 with 4 value heads, 2.3e-4 with 8 (bound 1e-3)."""
import functools

import numpy as np
import pytest

from tests.test_decode_gpu import build
from tests.test_multi_paged_gpu import _state_error
from tests.test_speculative_gpu import _same, _snap

pytestmark = pytest.mark.gpu
U = np.uint32
OPT = "multi_extend_la_chunk"
FLASH = "multi_extend_flash"
KV_MAX = 260
LA = ("la", "la")
HYBRID = ("la", "gqa", "la")
# (key heads, value heads): nv % 8 != 0 and == 0 are the two workgroup mappings of the scan; 1 and 4 value heads per key head
LA_HEADS = [(2, 4), (1, 8), (4, 16)]
# (tokens already in the slot, tokens of the run): exactly one sub-chunk from zero state; a last sub-chunk of one token; 2 + a partial sub-chunk of 2; 42; 8
CASES = [(0, 64), (5, 65), (37, 130), (37, 170), (3, 200)]
SLOTS = [5, 0, 7, 2, 6]                                                     # slot numbers do not follow the rows

_stores = []


@pytest.fixture(autouse=True)
def options_off_afterwards():
    yield
    for st in _stores:
        st.set_option(OPT, 0); st.set_option(FLASH, 0); st.set_option("multi_attn_fast", 0); st.set_attention_mode(False); st.set_prefill_chunk(0)


def _toks(rng, d, n):
    return [int(x) for x in rng.integers(0, d["V"], n)]


def _bits(x):
    return np.ascontiguousarray(x).view(U).copy()


def _pages(n, pt):
    return (n + pt - 1) // pt


@functools.lru_cache(maxsize=None)
def _model(kinds, la_heads=(2, 4), fp8=False, kv_max=KV_MAX, la_dkdv=(128, 128)):
    """one store per model, built once and shared"""
    st, eng, orc, keep, d = build(seed=3, hd=64, nh=4, kv_max=kv_max, kinds=list(kinds), la_heads=la_heads, la_dkdv=la_dkdv)
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
def _refs(kinds, la_heads, fp8=False):
    """the runs of CASES and their single-sequence references: computed once, shared by the tests, never modified"""
    st, _, d = _model(kinds, la_heads, fp8)
    rng = np.random.default_rng(7 + la_heads[1])
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


def _rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


# ---- 1: linear-attention stores: a run equals the single-sequence fast prompt pass, its neighbours the option-off call ----------------------------------------
def _crowded_call(st, d, refs, on):
    """the five runs of CASES, two unit rows and a run of 63 tokens in one extend_multi, slots scrambled; slots 4 and 9 hold state and are not in the call"""
    st.create_slots(10, KV_MAX)
    for ref, s in zip(refs, SLOTS):
        _fill(st, d, ref["prefix"], [s])
    _fill(st, d, refs[1]["prefix"], [3]); _fill(st, d, refs[2]["prefix"], [8, 4]); _fill(st, d, refs[4]["prefix"], [1, 9])
    slots = [3, SLOTS[0], SLOTS[1], 1, SLOTS[2], 8, SLOTS[3], SLOTS[4]]
    runs = [refs[1]["run"][:1], refs[0]["run"], refs[1]["run"], refs[4]["run"][:63], refs[2]["run"], refs[2]["run"][:1], refs[3]["run"], refs[4]["run"]]
    pos = [refs[1]["pos0"], refs[0]["pos0"], refs[1]["pos0"], refs[4]["pos0"], refs[2]["pos0"], refs[2]["pos0"], refs[3]["pos0"], refs[4]["pos0"]]
    st.set_option(OPT, on)
    ids, lg = st.extend_multi(slots, runs, pos, logits=True)
    st.set_option(OPT, 0)
    return slots, runs, pos, list(ids), lg


@pytest.mark.parametrize("la_heads", LA_HEADS)
def test_runs_equal_the_fast_prompt_pass_and_short_runs_keep_their_bits(la_heads):
    st, _, d = _model(LA, la_heads)
    refs = _refs(LA, la_heads)
    short = {0: 3, 3: 1, 5: 8}                                              # call row -> slot of the unit rows and the 63-token run
    slots, runs, pos, ids0, lg0 = _crowded_call(st, d, refs, 0)
    off = {r: _slot_state(st, d, s, pos[r] + len(runs[r])) for r, s in short.items()}
    idle = [_slot_state(st, d, 4, refs[2]["pos0"]), _slot_state(st, d, 9, refs[4]["pos0"])]
    slots, runs, pos, ids1, lg1 = _crowded_call(st, d, refs, 1)
    for row, case in ((1, 0), (2, 1), (4, 2), (6, 3), (7, 4)):
        _assert_run(st, d, refs[case], slots[row], ids1[row], lg1[row], ("case", case))
    for r, s in short.items():
        assert ids1[r] == ids0[r] and np.array_equal(_bits(lg1[r]), _bits(lg0[r])), ("short run", r)
        _same(_slot_state(st, d, s, pos[r] + len(runs[r])), off[r])
    _same(_slot_state(st, d, 4, refs[2]["pos0"]), idle[0]); _same(_slot_state(st, d, 9, refs[4]["pos0"]), idle[1])


# ---- 2: hybrid store with both options: the fast prefill, flat, paged and forked -------------------------------------------------------------------------------
@pytest.mark.parametrize("fp8", [False, True])
def test_hybrid_store_with_both_options_equals_the_fast_prefill(fp8):
    """37 tokens in the slot, a run of 170: logits, id, K / V rows, conv and recurrent state; a 63-token run beside it keeps the flash option's bits; then pages of
    32 positions and both dsts of a fork"""
    st, _, d = _model(HYBRID, (2, 4), fp8)
    ref = _refs(HYBRID, (2, 4), fp8)[3]
    for paged in (False, True):
        kw = dict(page_tokens=32, n_pages=4 * _pages(ref["end"], 32) + 2) if paged else {}
        st.create_slots(6, KV_MAX, **kw)
        _fill(st, d, ref["prefix"], [4, 2])
        st.set_option(OPT, 1); st.set_option(FLASH, 1)
        ids, lg = st.extend_multi([4], [ref["run"]], [ref["pos0"]], logits=True)
        _assert_run(st, d, ref, 4, ids[0], lg[0], ("paged" if paged else "flat"))
        if paged:
            src = _slot_state(st, d, 2, ref["pos0"])
            st.fork_slot(2, [0, 5], ref["pos0"])
            ids, lg = st.extend_multi([5, 0], [ref["run"], ref["run"]], [ref["pos0"]] * 2, logits=True)
            for r, s in enumerate([5, 0]):
                _assert_run(st, d, ref, s, ids[r], lg[r], ("fork dst", s))
            _same(_slot_state(st, d, 2, ref["pos0"]), src)                  # the fork's src is untouched
        st.set_option(OPT, 0); st.set_option(FLASH, 0)
    # every run of 2 .. 63 tokens equals the fast prefill too: the single-sequence fast pass keeps the exact rule below 64 tokens
    short = _fast_run(st, d, ref["prefix"], ref["run"][:63])
    st.create_slots(2, KV_MAX)
    _fill(st, d, ref["prefix"], [1])
    st.set_option(OPT, 1); st.set_option(FLASH, 1)
    ids, lg = st.extend_multi([1], [ref["run"][:63]], [ref["pos0"]], logits=True)
    st.set_option(OPT, 0); st.set_option(FLASH, 0)
    _assert_run(st, d, short, 1, ids[0], lg[0], "63 tokens")


# ---- 3: cuts ---------------------------------------------------------------------------------------------------------------------------------------------------
def _one_call(st, d, prefix, run, on, cuts=None):
    st.create_slots(2, KV_MAX)
    _fill(st, d, prefix, [1])
    st.set_option(OPT, on)
    p = len(prefix)
    for n in (cuts or [len(run)]):
        ids, lg = st.extend_multi([1], [run[p - len(prefix):p - len(prefix) + n]], [p], logits=True)
        p += n
    st.set_option(OPT, 0)
    return ids[0], lg[0].copy(), _slot_state(st, d, 1, p)


@pytest.mark.parametrize("la_heads", [(2, 4), (1, 8)])
def test_cuts_at_multiples_of_64_give_the_bits_of_one_call(la_heads):
    """192 tokens as 64 + 128 in two calls = one call: the state crosses a sub-chunk edge as the same f32 values through memory as through registers, and the prep
    of a sub-chunk depends on its own rows and the carried conv inputs only.  100 + 92 moves the sub-chunk edges: only the exact rule bounds it"""
    st, _, d = _model(LA, la_heads)
    rng = np.random.default_rng(31)
    prefix, run = _toks(rng, d, 5), _toks(rng, d, 192)
    one = _one_call(st, d, prefix, run, 1)
    two = _one_call(st, d, prefix, run, 1, [64, 128])
    assert two[0] == one[0] and np.array_equal(_bits(two[1]), _bits(one[1]))
    _same(two[2], one[2])
    exact = _one_call(st, d, prefix, run, 0)
    other = _one_call(st, d, prefix, run, 1, [100, 92])
    r = _rel(other[1], exact[1])
    print("multi_extend_la_chunk nv %d: 100 + 92 against exact %.3e, one call against exact %.3e (bound 1e-3)" % (la_heads[1], r, _rel(one[1], exact[1])))
    assert r <= 1e-3, r


# ---- 4: a full chunk -------------------------------------------------------------------------------------------------------------------------------------------
def test_full_chunk_of_1024_tokens():
    """one run of KR_EXTEND_MAX_TOKENS tokens at position 100 on the hybrid store, both options: 16 sub-chunks.  The store's fast prompt pass takes 1024 tokens as
    one chunk by default: its result is that of a pass told to use chunks of 1024"""
    st, _, d = _model(HYBRID, (2, 4), False, 1200)
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
    st.set_option(OPT, 1); st.set_option(FLASH, 1)
    ids, lg = st.extend_multi([1], [run], [100], logits=True)
    st.set_option(OPT, 0); st.set_option(FLASH, 0)
    _assert_run(st, d, ref, 1, ids[0], lg[0], "1024 tokens")


# ---- 5: the stated tolerances, option on against option off ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kinds,fp8,bound", [(LA, False, 1e-3), (HYBRID, False, 3e-3), (HYBRID, True, 3e-3)])
def test_on_against_off_within_the_stated_bound(kinds, fp8, bound):
    """LA-only: the bound of test_chunked_delta_rule_matches_exact_within_tolerance, 1e-3; hybrid store with this option alone (no single-sequence equal): the
    KR_ATTN_FAST prompt-pass bound, 3e-3 (docs/design/02-numerics.md 2b) -- on the run's last-token logits and on the next step_multi; the same greedy id"""
    st, _, d = _model(kinds, (2, 4), fp8)
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
    r_run, r_next = _rel(l1, l0), _rel(m1, m0)
    print("multi_extend_la_chunk %s %s: run %.3e  next step %.3e (bound %.0e)" % ("+".join(kinds), "E4M3" if fp8 else "FP16", r_run, r_next, bound))
    assert r_run <= bound and r_next <= bound, (r_run, r_next)
    assert t1 == t0 and n1 == n0


# ---- 6: what must not change -----------------------------------------------------------------------------------------------------------------------------------
def _unchanged_calls(st, d, refs, on):
    """step_multi, generate_multi, verify_multi + commit_multi with a rejected draft, generate_multi_lookup, an extend_multi of short runs only"""
    pick, slots = [1, 2, 4], [3, 0, 5]
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
    for i, s in zip(pick, twins):
        _fill(st, d, refs[i]["prefix"], [s])
    ids, lg = st.extend_multi(twins, [refs[i]["run"][:n] for i, n in zip(pick, (63, 2, 40))], pos, logits=True)
    out["short"] = (list(ids), _bits(lg))
    out["short_states"] = [_slot_state(st, d, s, p + n) for s, p, n in zip(twins, pos, (63, 2, 40))]
    st.set_option(OPT, 0)
    return out


def test_short_runs_and_verify_passes_keep_their_bits():
    st, _, d = _model(HYBRID, (2, 4), False)
    refs = _refs(HYBRID, (2, 4), False)
    off, on = _unchanged_calls(st, d, refs, 0), _unchanged_calls(st, d, refs, 1)
    assert on["step"][0] == off["step"][0] and np.array_equal(on["step"][1], off["step"][1])
    assert on["gen"] == off["gen"] and on["verify"] == off["verify"] and on["plain"] == off["plain"] and on["lookup"] == off["lookup"]
    assert on["short"][0] == off["short"][0] and np.array_equal(on["short"][1], off["short"][1])
    for a, b in zip(on["states"] + on["short_states"], off["states"] + off["short_states"]):
        _same(a, b)
    assert on["lookup"] == on["plain"]                                      # speculation stays exact under the option


# ---- 7: refusals, then option 0 --------------------------------------------------------------------------------------------------------------------------------
def _calls(st, V):
    t = lambda k: [x % V for x in range(1, 1 + k)]
    return (lambda: st.step_multi([1], t(1), [0]), lambda: st.extend_multi([1], [t(3)], [0]), lambda: st.generate_multi([1], t(1), [0], 2),
            lambda: st.verify_multi([1], [t(2)], [0]), lambda: st.generate_multi_lookup([1], t(1), [0], 2))


def test_store_without_linear_attention_layers_is_refused():
    st, _, d = _model(("gqa", "gqa"), kv_max=32)
    st.create_slots(2, 20)
    st.set_option(OPT, 1)
    for call in _calls(st, d["V"]):
        _state_error(call, OPT, "has none")
    st.set_option(OPT, 0)
    st.step_multi([1], [1], [0])


def test_mla_store_is_refused():
    from tests.test_mla_gpu import build as build_mla
    st, eng, orc, keep, d = build_mla(kv_max=24)
    _stores.append(st)
    st.create_slots(2, 20)
    st.set_option(OPT, 1)
    for call in _calls(st, d["V"]):
        _state_error(call, OPT)
    st.set_option(OPT, 0)
    st.step_multi([1], [1], [0])


def test_key_width_64_is_refused_not_run_exactly():
    st, _, d = _model(LA, (2, 4), False, 100, (64, 64))
    rng = np.random.default_rng(5)
    prefix, run = _toks(rng, d, 5), _toks(rng, d, 70)
    st.create_slots(2, 100)
    _fill(st, d, prefix, [1])
    before = _slot_state(st, d, 1, 5)
    st.set_option(OPT, 1)
    for call in list(_calls(st, d["V"])) + [lambda: st.extend_multi([1], [run], [5])]:
        with pytest.raises(ValueError) as e:
            call()
        assert OPT in str(e.value) and "not covered" in str(e.value), str(e.value)
    st.set_option(OPT, 0)                                                   # (load_slot is a slot call too: refused while the option stands)
    _same(_slot_state(st, d, 1, 5), before)                                 # nothing ran
    ids, lg = st.extend_multi([1], [run], [5], logits=True)                 # the slot the refusals left behind takes the exact pass
    got = (ids[0], lg[0].copy())
    want = _one_call(st, d, prefix, run, 0)
    assert got[0] == want[0] and np.array_equal(_bits(got[1]), _bits(want[1]))


def test_mode_bits_and_the_paged_refusal_come_first():
    st, _, d = _model(HYBRID, (2, 4), False)
    st.set_option(OPT, 1)
    st.create_slots(2, KV_MAX)
    st.set_attention_mode(True)
    for call in _calls(st, d["V"]):
        _state_error(call, "exact-mode only")
    st.set_attention_mode(False)
    # "multi_attn_fast" alone on paged slots is still refused with the words it had
    st.create_slots(2, 32, page_tokens=32, n_pages=2)
    st.set_option("multi_attn_fast", 1)
    for call in _calls(st, d["V"]):
        _state_error(call, "does not read paged slots")
    st.set_option("multi_attn_fast", 0)
    st.set_option(OPT, 0)
