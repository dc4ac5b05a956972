"""The "multi_mla_fast" option of the batched multi-sequence decode (docs/design/24-multi-mla-fast.md): with it set, the MLA layers of every batched
entry point run split-KV flash-decode over the rows' slots, flat or paged.  Over slots longer than mla_split_min (512) row i is BIT-IDENTICAL to the
single-sequence fast step -- decode_step under set_attention_mode(True) on a store whose kv_max_seq is above 512 -- on that sequence alone: logits, id,
the latent and rope-key rows it appends, whatever rows share the launch, whatever the slot capacity, page size, page placement or sharing by fork, with
FP16 and E4M3 caches.  Over shorter slots the step is the exact one, bit for bit.  Against the exact batched step the logits stay within the project's
bound for this operator (docs/design/02-numerics.md section 2b, tests/test_attn_fast_gpu.py: max |on - off| <= 3e-3 max |off| with FP16 caches, 5e-3 with
E4M3).  The reference everywhere is the single-sequence fast step or the option-off step; the option-on path is never compared with itself."""
import functools

import numpy as np
import pytest

import tests.test_multi_mla_gpu as MM
from tests.test_multi_paged_gpu import Mla, _slot_state, _state_error, _toks

pytestmark = pytest.mark.gpu
F = np.float32
U = np.uint32
OPT = "multi_mla_fast"

KV_MAX = 700                                     # the store's kv_max_seq: above mla_split_min, 64-position chunks
# (kv_lora_rank, heads, LoRA query path, E4M3 caches); 64 heads fill the query tile exactly
MODELS = [(512, 5, False, False), (256, 3, False, True), (512, 64, True, True)]
A, B, C = MODELS
# one position | a full 32-position tile and the position after it | a full 64-position chunk and a chunk of one position | several chunks, ragged tail
LENS = (0, 31, 32, 63, 64, 300, 650)
LONG = LENS.index(650)
N_STEPS = 3

_stores = []


@pytest.fixture(autouse=True)
def options_off_afterwards():
    yield
    for st in _stores:
        st.set_option(OPT, 0); st.set_option("multi_attn_fast", 0); st.set_option("multi_attn_fast_paged", 0); st.set_attention_mode(False)


def _bits(lg):
    return lg.view(U).copy()


def _pages(n, pt):
    return (n + pt - 1) // pt


def _start(st, d, prompt):
    """the store's own sequence = prompt, by the EXACT prompt pass (zero state first)"""
    st.set_attention_mode(False)
    MM._start(st, d, prompt)


def _fast_steps(st, d, prompt, tokens):
    """exact prompt pass, then decode_step under KR_ATTN_FAST over `tokens`: per step (logits bits, greedy id); the state snapshot after the steps"""
    _start(st, d, prompt)
    st.set_attention_mode(True)
    try:
        out, pos = [], len(prompt)
        for tok in tokens:
            st.decode_step(tok, pos)
            out.append((_bits(st.read_logits()), st.last_token())); pos += 1
        snap = MM._snap(st, d, pos)
    finally:
        st.set_attention_mode(False)
    return out, snap


def _fast_reference(st, d, prompt, first, n_steps):
    """the same, feeding each step's greedy id to the next"""
    _start(st, d, prompt)
    st.set_attention_mode(True)
    try:
        out, tok, pos = [], first, len(prompt)
        for _ in range(n_steps):
            st.decode_step(tok, pos)
            out.append((_bits(st.read_logits()), st.last_token()))
            tok = out[-1][1]; pos += 1
        snap = MM._snap(st, d, pos)
    finally:
        st.set_attention_mode(False)
    return out, snap


def _fill_slots(st, d, prompts, slot_lists):
    for p, slots in zip(prompts, slot_lists):
        _start(st, d, p)
        for s in slots:
            st.save_slot(s, len(p))


@functools.lru_cache(maxsize=None)
def _model(klr, nh, lora, fp8, kv_max=KV_MAX, lens=LENS, n_steps=N_STEPS):
    """one store per geometry, its sequences and their single-sequence fast references: computed once, shared by the tests, never modified"""
    st, eng, keep, d = MM._build(fp8, seed=3, klr=klr, nh=nh, lora=lora, kv_max=kv_max)
    _stores.append(st)
    rng = np.random.default_rng(klr + nh)
    prompts = [MM._prompt(rng, d, n) for n in lens]
    firsts = [int(x) for x in rng.integers(0, d["V"], len(prompts))]
    refs = [_fast_reference(st, d, p, f, n_steps) for p, f in zip(prompts, firsts)]
    return st, (eng, keep), d, prompts, firsts, refs


def _steps_against_refs(st, slots, firsts, refs, lens, n_steps=N_STEPS):
    toks, pos = list(firsts), list(lens)
    for k in range(n_steps):
        ids, lg = st.step_multi(slots, toks, pos, logits=True)
        for i, (ref, _) in enumerate(refs):
            assert np.array_equal(lg[i].view(U), ref[k][0]), ("logits", k, lens[i])
            assert ids[i] == ref[k][1], ("id", k, lens[i])
        toks = [ref[k][1] for ref, _ in refs]; pos = [p + 1 for p in pos]
    return pos


# ---- 1: rows equal the single-sequence fast step ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("slot_seq", [700, 1000])
@pytest.mark.parametrize("key", MODELS)
def test_row_equals_single_sequence_fast_step(key, slot_seq):
    st, _, d, prompts, firsts, refs = _model(*key)
    slots = [4, 0, 6, 2, 7, 1, 5]                                           # scrambled: slot numbers need not follow the rows
    st.create_slots(8, slot_seq)
    _fill_slots(st, d, prompts, [[s] for s in slots])
    st.set_option(OPT, 1)
    pos = _steps_against_refs(st, slots, firsts, refs, LENS)
    st.set_option(OPT, 0)
    for i, (_, snap) in enumerate(refs):
        MM._same(_slot_state(Mla, st, d, slots[i], pos[i]), snap)


# ---- 2: batch composition -----------------------------------------------------------------------------------------------------------------------------------
def _composition(st, d, prompts, firsts, refs, **paged):
    others = [i for i in range(len(LENS)) if i != LONG]
    n_other = 32
    per_seq = [[] for _ in LENS]
    per_seq[LONG] = [0, 1, 2, 3]
    groups = []
    for g in range(3):
        rows = []
        for r in range(n_other):
            q = others[r % len(others)]; s = 4 + g * n_other + r
            per_seq[q].append(s); rows.append((q, s))
        groups.append(rows)
    if paged:
        paged["n_pages"] = sum(_pages(LENS[q] + 1, paged["page_tokens"]) * len(s) for q, s in enumerate(per_seq))
    st.create_slots(4 + 3 * n_other, KV_MAX, **paged)
    _fill_slots(st, d, prompts, per_seq)
    st.set_option(OPT, 1)
    batches = [[(LONG, 0)], [(LONG, 1)] + groups[0], groups[1] + [(LONG, 2)]]
    rng = np.random.default_rng(4)
    batches.append([(groups[2] + [(LONG, 3)])[j] for j in rng.permutation(n_other + 1)])
    for rows in batches:
        ids, lg = st.step_multi([s for _, s in rows], [firsts[q] for q, _ in rows], [len(prompts[q]) for q, _ in rows], logits=True)
        for r, (q, _) in enumerate(rows):
            assert np.array_equal(lg[r].view(U), refs[q][0][0][0]), (len(rows), r, LENS[q])
            assert ids[r] == refs[q][0][0][1], (len(rows), r, LENS[q])


@pytest.mark.parametrize("page_tokens", [0, 64])
def test_batch_composition(page_tokens):
    """the 650-position sequence alone, as row 0 and as row 32 of a 33-row batch of other lengths (this crosses the 32-row switch of the matrix-core
    absorption and w_vc forms), and in a permuted batch: the same bits.  The grid's chunk count follows the longest row; the workgroups of shorter rows
    past their end leave"""
    st, _, d, prompts, firsts, refs = _model(*A)
    _composition(st, d, prompts, firsts, refs, **(dict(page_tokens=page_tokens) if page_tokens else {}))


# ---- 3: paged slots -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("page_tokens", [32, 64, 256])
@pytest.mark.parametrize("key", MODELS)
def test_paged_row_equals_single_sequence_fast_step(key, page_tokens):
    """page_tokens 32: a tile is a page and a chunk two; 64: a chunk is a page; 256: four chunks share a page and in-page offsets reach 255.  Rows in
    scrambled slot order; the longest row's pages are not contiguous: a spare slot saved between the fills leaves a hole that row takes first.  The
    references are those of the flat test, so paged rows carry the bits of flat rows under the option"""
    st, _, d, prompts, firsts, refs = _model(*key)
    pt = page_tokens
    slots, spare = [4, 0, 6, 2, 7, 1, 5], 3
    st.create_slots(8, KV_MAX, page_tokens=pt, n_pages=sum(_pages(n + N_STEPS, pt) for n in LENS) + 2)
    _fill_slots(st, d, prompts[:5], [[s] for s in slots[:5]])
    st.save_slot(spare, 40)                                                 # pages between the short rows and the 300-position row ...
    _fill_slots(st, d, prompts[5:6], [[slots[5]]])
    st.trim_slot(spare, 0)                                                  # ... come back as a hole: lowest free id first hands it to the longest row
    _fill_slots(st, d, prompts[6:], [[slots[6]]])
    used = st.slot_page_ids(slots[LONG])[0][:_pages(LENS[LONG], pt)]
    assert min(used) >= 0 and len(set(np.diff(used).tolist())) > 1, ("the longest row's pages are an arithmetic progression", used)
    st.set_option(OPT, 1)
    pos = _steps_against_refs(st, slots, firsts, refs, LENS)
    st.set_option(OPT, 0)
    for i, (_, snap) in enumerate(refs):
        MM._same(_slot_state(Mla, st, d, slots[i], pos[i]), snap)


def _fork_run(st, d, paged, pt, prompts, firsts, toks, new):
    SRC, DSTS, FORK, REWIND = 3, [0, 2], 600, 500
    st.set_option(OPT, 0)
    st.create_slots(4, KV_MAX, **(dict(page_tokens=pt, n_pages=_pages(651, pt) + 2 + _pages(602, pt) - FORK // pt + 2) if paged else {}))
    _fill_slots(st, d, [prompts[LONG]], [[SRC]])
    st.fork_slot(SRC, DSTS, FORK)
    full = FORK // pt
    if paged:
        tables = [st.slot_page_ids(s) for s in [SRC] + DSTS]
        for ids, refc in tables:
            assert ids[:full] == tables[0][0][:full] and refc[:full] == [3] * full      # whole pages shared by the three slots
        assert len({ids[full] for ids, _ in tables}) == 3 and all(refc[full] == 1 for _, refc in tables)      # a private boundary page each
    st.set_option(OPT, 1)
    out = []
    ids, lg = st.step_multi(DSTS, toks[:2], [FORK, FORK], logits=True)     # each destination with its own first token
    out.append((list(ids), _bits(lg)))
    ids, lg = st.extend_multi([DSTS[0]], [new], [REWIND], logits=True)      # a write below the fork point: copy-on-write of the pages it lands in
    out.append((list(ids), _bits(lg)))
    if paged:
        ids_d, refc = st.slot_page_ids(DSTS[0])
        hit = range(REWIND // pt, _pages(REWIND + len(new), pt))
        assert all(refc[j] == 1 and ids_d[j] != tables[0][0][j] for j in hit) and all(st.slot_page_ids(SRC)[1][j] == 2 for j in hit)
    ids, lg = st.step_multi([SRC] + DSTS, [firsts[LONG], toks[2], toks[3]], [650, REWIND + len(new), FORK + 1], logits=True)
    out.append((list(ids), _bits(lg)))
    st.set_option(OPT, 0)
    return out, [_slot_state(Mla, st, d, s, n) for s, n in ((SRC, 651), (DSTS[0], REWIND + len(new) + 1), (DSTS[1], FORK + 2))]


@pytest.mark.parametrize("page_tokens", [32, 64])
def test_forked_slots(page_tokens):
    """the 650-position slot forked at 600 to two destinations: whole pages shared, a private boundary page each; a step of each destination with its own
    token, a rewind of one by extend_multi from position 500 (copy-on-write), a step of all three.  Equal to flat forked slots under the option; the
    source's step also equals the single-sequence fast reference"""
    st, _, d, prompts, firsts, refs = _model(*A)
    rng = np.random.default_rng(8)
    toks, new = _toks(rng, d, 4), _toks(rng, d, 20)
    got, states = _fork_run(st, d, True, page_tokens, prompts, firsts, toks, new)
    flat, flat_states = _fork_run(st, d, False, page_tokens, prompts, firsts, toks, new)
    for (ids, lg), (fids, flg) in zip(got, flat):
        assert ids == fids and np.array_equal(lg, flg)
    for a, b in zip(states, flat_states):
        MM._same(a, b)
    assert np.array_equal(got[2][1][0], refs[LONG][0][0][0]) and got[2][0][0] == refs[LONG][0][0][1]


def _poison(st, d, n):
    """the store's own sequence = n rows of 0xFF bytes in both caches of every layer (NaN patterns in FP16 and in E4M3)"""
    t = np.uint8 if d["fp8"] else np.uint16
    ck = [np.full((d["kv_max"], d["klr"]), np.iinfo(t).max, t) for _ in range(d["nL"])]
    kp = [np.full((d["kv_max"], d["rd"]), np.iinfo(t).max, t) for _ in range(d["nL"])]
    z = [0] * d["nL"]
    st.set_decode_state(n, d["kv_max"], z, z, z, z, [x.ctypes.data for x in ck], [x.ctypes.data for x in kp])
    return ck, kp


@pytest.mark.parametrize("page_tokens", [0, 32])
@pytest.mark.parametrize("key", [A, B])
def test_rows_past_the_length_do_not_leak_in(key, page_tokens):
    """every slot first holds 690 rows of 0xFF bytes, then its sequence is saved over the head of them: the rows past its length -- the rest of its last
    page, and on flat slots of its capacity -- are NaN patterns.  The whole pages past the length go back to the pool dirty (trim) and are handed out
    again.  Two slots also hold the rejected draft rows of a verify that kept nothing.  The next steps still equal the single-sequence reference"""
    st, _, d, prompts, firsts, refs = _model(*key)
    pt = page_tokens
    n = len(LENS)
    st.create_slots(n, KV_MAX, **(dict(page_tokens=pt, n_pages=n * _pages(690, pt)) if pt else {}))
    keep = _poison(st, d, 690)
    for s in range(n):
        st.save_slot(s, 690)
    _fill_slots(st, d, prompts, [[s] for s in range(n)])                    # rows [0, len) of each slot; the rest keeps the 0xFF bytes
    if pt:
        for s in range(n):
            st.trim_slot(s, LENS[s])
        assert st.slot_pages()["per_slot"] == [_pages(m, pt) for m in LENS]
    del keep
    st.set_option(OPT, 1)
    rng = np.random.default_rng(5)
    i63, i300 = LENS.index(63), LENS.index(300)
    st.verify_multi([i63, i300], [[firsts[i63]] + _toks(rng, d, 4), [firsts[i300]] + _toks(rng, d, 15)], [63, 300])
    st.commit_multi([0, 0])
    _steps_against_refs(st, list(range(n)), firsts, refs, LENS)


def test_pool_one_page_short_fails_whole():
    """two rows that each need one more page where one is free: refused whole with the option on, pages and slots unchanged; a call that fits runs"""
    st, _, d, prompts, firsts, refs = _model(*A)
    pt = 32
    i32, i64 = LENS.index(32), LENS.index(64)
    st.create_slots(2, KV_MAX, page_tokens=pt, n_pages=_pages(32, pt) + _pages(64, pt) + 1)
    _fill_slots(st, d, [prompts[i32], prompts[i64]], [[0], [1]])
    before = st.slot_pages()
    assert before["free"] == 1
    want = [_slot_state(Mla, st, d, 0, 32), _slot_state(Mla, st, d, 1, 64)]
    st.set_option(OPT, 1)
    _state_error(lambda: st.step_multi([0, 1], [firsts[i32], firsts[i64]], [32, 64]), "row 1", "slot 1")
    _state_error(lambda: st.extend_multi([0, 1], [[1, 2], [3, 4]], [32, 64]), "row 1", "slot 1")
    assert st.slot_pages() == before
    st.set_option(OPT, 0)
    MM._same(_slot_state(Mla, st, d, 0, 32), want[0]); MM._same(_slot_state(Mla, st, d, 1, 64), want[1])
    st.set_option(OPT, 1)
    ids, lg = st.step_multi([1], [firsts[i64]], [64], logits=True)
    assert np.array_equal(lg[0].view(U), refs[i64][0][0][0]) and ids[0] == refs[i64][0][0][1]


# ---- 4: every entry point once ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("page_tokens", [0, 32])
def test_every_entry_point_equals_that_many_fast_steps(page_tokens):
    st, _, d, prompts, firsts, refs = _model(*B)
    pt = page_tokens
    rng = np.random.default_rng(6)
    i63, i300 = LENS.index(63), LENS.index(300)
    # extend_multi: runs of 1, 17 (over the chunk edge at 64) and 40 tokens (over the chunk edge at 320)
    runs = [[firsts[LONG]], [firsts[i63]] + _toks(rng, d, 16), [firsts[i300]] + _toks(rng, d, 39)]
    seqs = [LONG, i63, i300]
    want = [_fast_steps(st, d, prompts[q], run) for q, run in zip(seqs, runs)]
    fresh = _toks(rng, d, 100)
    want_fresh = _fast_steps(st, d, [], fresh)
    # verify: the 300-position row's own greedy continuation and then a wrong token -- one draft accepted, one rejected; two tokens kept
    vrun = [firsts[i300], refs[i300][0][0][1], (refs[i300][0][1][1] + 1) % d["V"]]
    want_v = _fast_steps(st, d, prompts[i300], vrun[:2])

    def single(q, max_tokens):
        _start(st, d, prompts[q])
        st.set_attention_mode(True)
        try:
            out = st.generate_batch(firsts[q], LENS[q], max_tokens)
            return out, MM._snap(st, d, LENS[q] + len(out))
        finally:
            st.set_attention_mode(False)

    want_g = [single(q, 5) for q in (LONG, i63)]
    st.create_slots(8, KV_MAX, **(dict(page_tokens=pt, n_pages=3 * _pages(660, pt) + 3 * _pages(350, pt) + 2 * _pages(110, pt)) if pt else {}))
    _fill_slots(st, d, [prompts[LONG], prompts[i63], prompts[i300]], [[0, 5], [1, 6], [2, 3]])
    st.set_option(OPT, 1)
    ids, lg = st.extend_multi([0, 1, 2], runs, [LENS[q] for q in seqs], logits=True)
    for r, (steps, _) in enumerate(want):
        assert np.array_equal(lg[r].view(U), steps[-1][0]) and ids[r] == steps[-1][1], ("extend", r)
    assert st.prefill_slot(4, fresh, 0, chunk=33) == want_fresh[0][-1][1]
    greedy, nm = st.verify_multi([3], [vrun], [300])
    assert list(nm) == [1] and list(greedy[0][:2]) == [s[1] for s in want_v[0]]
    st.commit_multi([2])
    out = st.generate_multi([5, 6], [firsts[LONG], firsts[i63]], [LENS[LONG], LENS[i63]], 5)
    assert out == [T for T, _ in want_g]
    st.set_option(OPT, 0)
    ends = [LENS[q] + len(run) for q, run in zip(seqs, runs)]
    for r, (_, snap) in enumerate(want):
        MM._same(_slot_state(Mla, st, d, r, ends[r]), snap)
    MM._same(_slot_state(Mla, st, d, 4, 100), want_fresh[1])
    MM._same(_slot_state(Mla, st, d, 3, 302), want_v[1])
    for s, q, (T, snap) in zip((5, 6), (LONG, i63), want_g):
        MM._same(_slot_state(Mla, st, d, s, LENS[q] + len(T)), snap)
    # the lookup loop: the same tokens as the plain loop, from fresh copies of the two slots
    _fill_slots(st, d, [prompts[LONG], prompts[i63]], [[5], [6]])
    st.set_option(OPT, 1)
    out = st.generate_multi_lookup([5, 6], [firsts[LONG], firsts[i63]], [LENS[LONG], LENS[i63]], 5, [prompts[LONG], prompts[i63]], 4, 2)
    assert out == [T for T, _ in want_g]
    st.set_option(OPT, 0)
    for s, q, (T, snap) in zip((5, 6), (LONG, i63), want_g):
        MM._same(_slot_state(Mla, st, d, s, LENS[q] + len(T)), snap)


# ---- 5: chunks of 128 positions -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("page_tokens", [0, 32])
def test_chunk_of_128_positions(page_tokens):
    """a store and slots of 16 500 positions: a chunk is 128 positions (four tiles, four table entries at page_tokens 32).  Rows of 200 positions (two
    chunks, a ragged tail) and 130 (a chunk of two positions) against the store's own fast step"""
    kv_max, lens = 16500, (200, 130)
    st, _, d, prompts, firsts, refs = _model(*A, kv_max=kv_max, lens=lens, n_steps=2)
    pt = page_tokens
    st.create_slots(3, kv_max, **(dict(page_tokens=pt, n_pages=_pages(202, pt) + _pages(132, pt) + 2) if pt else {}))
    _fill_slots(st, d, prompts[:1], [[2]])
    st.save_slot(1, 40)
    _fill_slots(st, d, prompts[1:], [[0]])
    st.set_option(OPT, 1)
    pos = _steps_against_refs(st, [2, 0], firsts, refs, lens, 2)
    st.set_option(OPT, 0)
    for i, s in enumerate((2, 0)):
        MM._same(_slot_state(Mla, st, d, s, pos[i]), refs[i][1])


# ---- 6: short slots -----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("page_tokens", [0, 32])
def test_short_slots_keep_the_exact_step(page_tokens):
    """slots of max_seq 512 = mla_split_min: the capacity rule of the store's own fast step -- the exact per-slot kernel, the option-off bits"""
    st, _, d, prompts, firsts, refs = _model(*A)
    pt = page_tokens
    short = [i for i, n in enumerate(LENS) if n <= 300]
    n = len(short)
    st.create_slots(2 * n, 512, **(dict(page_tokens=pt, n_pages=2 * sum(_pages(LENS[i] + N_STEPS, pt) for i in short)) if pt else {}))
    _fill_slots(st, d, [prompts[i] for i in short], [[j, n + j] for j in range(n)])
    runs = []
    for on, base in ((0, 0), (1, n)):
        st.set_option(OPT, on)
        toks, pos, out = [firsts[i] for i in short], [LENS[i] for i in short], []
        for _ in range(N_STEPS):
            ids, lg = st.step_multi(list(range(base, base + n)), toks, pos, logits=True)
            out.append((ids, _bits(lg))); toks = ids; pos = [p + 1 for p in pos]
        runs.append(out)
    for (ids0, lg0), (ids1, lg1) in zip(*runs):
        assert ids0 == ids1 and np.array_equal(lg0, lg1)
    st.set_option(OPT, 0)
    for j, i in enumerate(short):
        MM._same(_slot_state(Mla, st, d, j, LENS[i] + N_STEPS), _slot_state(Mla, st, d, n + j, LENS[i] + N_STEPS))


# ---- 7: the stated tolerance against the exact batched step -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", MODELS)
def test_within_stated_tolerance_of_the_exact_batched_step(key):
    """STATED TOLERANCE (02-numerics.md section 2b, tests/test_attn_fast_gpu.py): max |on - off| <= 3e-3 max |off| (FP16 caches) / 5e-3 (E4M3) on every
    row's logits, same greedy ids; rows of 300 positions or more differ from the exact bits somewhere (no silent fall-back to the exact kernel).
    Largest ratio observed on an MI355X: 9.98e-4 (klr 512, nh 5, FP16), 2.85e-3 (klr 256, nh 3, E4M3), 2.20e-3 (klr 512, nh 64, LoRA, E4M3)"""
    st, _, d, prompts, firsts, refs = _model(*key)
    bound = 5e-3 if key[3] else 3e-3
    n = len(LENS)
    st.create_slots(2 * n, KV_MAX)
    _fill_slots(st, d, prompts, [[i, n + i] for i in range(n)])
    toks, pos, exact = list(firsts), list(LENS), []
    for k in range(N_STEPS):
        ids, lg = st.step_multi(list(range(n)), toks, pos, logits=True)
        exact.append((toks, ids, lg)); toks = ids; pos = [p + 1 for p in pos]
    st.set_option(OPT, 1)
    pos, worst, differs = list(LENS), 0.0, False
    for k, (fed, ids_e, lg_e) in enumerate(exact):
        ids, lg = st.step_multi(list(range(n, 2 * n)), fed, pos, logits=True)
        for i in range(n):
            worst = max(worst, float(np.abs(lg[i] - lg_e[i]).max() / np.abs(lg_e[i]).max()))
            if LENS[i] >= 300:
                differs |= not np.array_equal(lg[i].view(U), lg_e[i].view(U))
        print(f"klr {key[0]} nh {key[1]} fp8 {key[3]} step {k}: largest max|on - off| / max|off| so far {worst:.3e} (bound {bound:.0e})")
        for i in range(n):
            assert float(np.abs(lg[i] - lg_e[i]).max()) <= bound * float(np.abs(lg_e[i]).max()), (k, LENS[i])
        assert ids == ids_e, k
        pos = [p + 1 for p in pos]
    assert differs, "no long row differs from the exact step in its bits: the flash-decode did not run"


# ---- 8: refusals and unchanged behaviour --------------------------------------------------------------------------------------------------------------------
def _calls(st, s, pos):
    return (lambda: st.step_multi([s], [2], [pos]), lambda: st.generate_multi([s], [2], [pos], 2), lambda: st.step_multi_sample([s], [2], [pos]),
            lambda: st.extend_multi([s], [[1, 2]], [pos]), lambda: st.verify_multi([s], [[2, 3]], [pos]), lambda: st.generate_multi_lookup([s], [2], [pos], 2),
            lambda: st.generate_multi([s], [2], [pos], 2, temperature=0.6, rng_seeds=3))


def test_a_store_without_mla_layers_is_refused():
    """an option that silently does nothing is a trap: on a GQA + linear-attention store every batched call raises KR_ERR_STATE naming the option"""
    from tests.test_multi_paged_gpu import Gqa
    st, keep, d = Gqa.build(False, seed=3, kv_max=48)
    _stores.append(st)
    rng = np.random.default_rng(3)
    prompt = _toks(rng, d, 20)
    Gqa.start(st, d, prompt)
    st.create_slots(2, 40, page_tokens=32, n_pages=4)
    st.save_slot(1, 20)
    want = _slot_state(Gqa, st, d, 1, 20)
    before = st.slot_pages()
    st.decode_step(5, 20)
    want_lg, want_tok = _bits(st.read_logits()), st.last_token()
    st.set_option(OPT, 1)
    for call in _calls(st, 1, 20):
        _state_error(call, OPT)
        assert np.array_equal(st.read_logits().view(U), want_lg) and st.last_token() == want_tok
        assert st.slot_pages() == before
    st.set_option(OPT, 0)
    Gqa.same(_slot_state(Gqa, st, d, 1, 20), want)
    st.step_multi([1], [2], [20])


def test_more_than_64_heads_are_refused():
    """65 heads: the single-sequence launcher keeps the exact kernels there, so there is no fast step to equal -- KR_ERR_VALUE naming the option"""
    st, eng, keep, d = MM._build(kv_max=48, nh=65)
    _stores.append(st)
    rng = np.random.default_rng(3)
    prompt = MM._prompt(rng, d, 20)
    ref, _ = MM._reference(st, d, prompt, 2, 1)
    st.create_slots(2, 40, page_tokens=32, n_pages=4)
    MM._fill_slots(st, d, [prompt], [[1]])
    want = _slot_state(Mla, st, d, 1, 20)
    before = st.slot_pages()
    st.decode_step(5, 20)
    want_lg, want_tok = _bits(st.read_logits()), st.last_token()
    st.set_option(OPT, 1)
    for call in _calls(st, 1, 20):
        with pytest.raises(ValueError, match=OPT):
            call()
        assert np.array_equal(st.read_logits().view(U), want_lg) and st.last_token() == want_tok
        assert st.slot_pages() == before
    st.set_option(OPT, 0)
    MM._same(_slot_state(Mla, st, d, 1, 20), want)
    ids, lg = st.step_multi([1], [2], [20], logits=True)
    assert np.array_equal(lg[0].view(U), ref[0][0]) and ids[0] == ref[0][1]


def test_other_refusals_stay_and_the_option_is_isolated():
    """the two GQA options on an MLA store keep their refusal and message with the new option set; the mode bits stay refused; nothing changes; the store's
    own exact step keeps its bits with the option set; option 0 afterwards gives the exact step's bits"""
    st, _, d, prompts, firsts, refs = _model(*A)
    i = LENS.index(300)
    _start(st, d, prompts[i])
    st.decode_step(firsts[i], 300)                                          # exact single-sequence step: the reference of the option-off step below
    exact_lg, exact_tok = _bits(st.read_logits()), st.last_token()
    st.create_slots(2, KV_MAX, page_tokens=32, n_pages=2 * _pages(310, 32))
    _fill_slots(st, d, [prompts[i]], [[0, 1]])
    want = _slot_state(Mla, st, d, 0, 300)
    before = st.slot_pages()
    st.decode_step(9, 300)
    want_lg, want_tok = _bits(st.read_logits()), st.last_token()
    st.set_option(OPT, 1)

    def unchanged():
        assert np.array_equal(st.read_logits().view(U), want_lg) and st.last_token() == want_tok
        assert st.slot_pages() == before

    for name in ("multi_attn_fast", "multi_attn_fast_paged"):
        st.set_option(name, 1)
        for call in _calls(st, 0, 300):
            _state_error(call, '"%s" option covers GQA layers only' % name)
            unchanged()
        st.set_option(name, 0)
    for bits in [dict(fast=True), dict(fast=False, gemm_fast=True), dict(fast=False, decode_fast=True)]:
        st.set_attention_mode(**bits)
        for call in _calls(st, 0, 300):
            _state_error(call, "exact-mode only")
            unchanged()
        st.set_attention_mode(False)
    st.set_option(OPT, 0)
    for s in (0, 1):
        MM._same(_slot_state(Mla, st, d, s, 300), want)
    st.set_option(OPT, 1)
    # the option touches the batched calls only: the store's own exact step and prompt pass keep their bits with it set
    _start(st, d, prompts[i])
    st.decode_step(firsts[i], 300)
    assert np.array_equal(st.read_logits().view(U), exact_lg) and st.last_token() == exact_tok
    ids, lg = st.step_multi([0], [firsts[i]], [300], logits=True)           # option on: the single-sequence FAST bits
    assert np.array_equal(lg[0].view(U), refs[i][0][0][0]) and ids[0] == refs[i][0][0][1]
    st.set_option(OPT, 0)
    ids, lg = st.step_multi([1], [firsts[i]], [300], logits=True)           # option off again: the exact bits
    assert np.array_equal(lg[0].view(U), exact_lg) and ids[0] == exact_tok
