"""The "multi_attn_fast" option of the batched multi-sequence decode (docs/design/16-multi-attn-fast.md): with it set, the GQA layers of every
batched step run split-KV flash-decode over the rows' slots.  Over slots longer than gqa_split_min (1024) row i of a step is BIT-IDENTICAL to the
single-sequence fast step -- decode_step under set_attention_mode(True) on a store whose kv_max_seq is above 1024 -- on that sequence alone:
logits, id, the K / V rows it appends, conv and recurrent state, whatever rows share the step, whatever the slot capacity.  Over shorter slots the
step is the exact one, bit for bit.  Against the exact batched step the logits stay within the project's bound for GQA flash-decode
(docs/design/02-numerics.md section 2b: max |fast - exact| <= 1e-3 max |exact|).  The reference everywhere is the single-sequence path or the
option-off step; the option-on step is never compared with itself."""
import functools

import numpy as np
import pytest

from tests.test_decode_gpu import build
from tests.test_speculative_gpu import _same, _snap

pytestmark = pytest.mark.gpu
F = np.float32
U = np.uint32

KV_MAX = 1300                                    # the store's kv_max_seq: above gqa_split_min, so its own fast step takes the flash-decode
MODELS = [(256, 16, False), (128, 8, True), (64, 4, False)]
# one position | a full 64-position tile and the position after it | a full 128-position chunk and a chunk of one position | several chunks, ragged tail
LENS = (0, 63, 64, 127, 128, 700, 1150)
N_STEPS = 3


def _prompt(rng, d, n):
    return [int(x) for x in rng.integers(0, d["V"], n)]


def _start(st, d, prompt):
    """the store's own sequence = prompt, by the EXACT prompt pass (zero state first)"""
    st.set_attention_mode(False)
    st.reset_decode_state(d["kv_max"])
    if prompt:
        st.prefill(prompt, 0)


def _fast_reference(st, d, prompt, first, n_steps):
    """exact prompt pass, then decode_step under KR_ATTN_FAST: per step (logits bits, greedy id); the state snapshot after the steps"""
    _start(st, d, prompt)
    st.set_attention_mode(True)
    try:
        out, tok, pos = [], first, len(prompt)
        for _ in range(n_steps):
            st.decode_step(tok, pos)
            out.append((st.read_logits().view(U).copy(), st.last_token()))
            tok = out[-1][1]; pos += 1
        snap = _snap(st, d, pos)
    finally:
        st.set_attention_mode(False)
    return out, snap


def _fill_slots(st, d, prompts, slot_lists):
    for p, slots in zip(prompts, slot_lists):
        _start(st, d, p)
        for s in slots:
            st.save_slot(s, len(p))


@functools.lru_cache(maxsize=None)
def _model(hd, nh, fp8):
    """one store per geometry, its sequences and their single-sequence fast references: computed once, shared by the tests, never modified"""
    st, eng, orc, keep, d = build(seed=3, hd=hd, nh=nh, kv_max=KV_MAX)
    if fp8:
        st.set_kv_dtype(True); d["fp8"] = True
    rng = np.random.default_rng(hd + nh)
    prompts = [_prompt(rng, d, n) for n in LENS]
    firsts = [int(x) for x in rng.integers(0, d["V"], len(prompts))]
    refs = [_fast_reference(st, d, p, f, N_STEPS) for p, f in zip(prompts, firsts)]
    return st, (eng, orc, keep), d, prompts, firsts, refs


@pytest.fixture
def option_off_afterwards():
    yield
    for key in MODELS:
        if key in _built:
            st = _model(*key)[0]
            st.set_option("multi_attn_fast", 0); st.set_attention_mode(False)


_built = set()


def _get(hd, nh, fp8):
    _built.add((hd, nh, fp8))
    return _model(hd, nh, fp8)


@pytest.mark.parametrize("slot_seq", [1200, 1500])
@pytest.mark.parametrize("hd,nh,fp8", MODELS)
def test_row_equals_single_sequence_fast_step(hd, nh, fp8, slot_seq, option_off_afterwards):
    st, _, d, prompts, firsts, refs = _get(hd, nh, fp8)
    slots = [4, 0, 6, 2, 7, 1, 5]                                           # scrambled: slot numbers need not follow the rows
    st.create_slots(8, slot_seq)
    _fill_slots(st, d, prompts, [[s] for s in slots])
    st.set_option("multi_attn_fast", 1)
    toks, pos = list(firsts), [len(p) for p in prompts]
    for k in range(N_STEPS):
        ids, lg = st.step_multi(slots, toks, pos, logits=True)
        for i, (ref, _) in enumerate(refs):
            assert np.array_equal(lg[i].view(U), ref[k][0]), ("logits", k, LENS[i])
            assert ids[i] == ref[k][1], ("id", k, LENS[i])
        toks = [ref[k][1] for ref, _ in refs]; pos = [p + 1 for p in pos]
    st.set_option("multi_attn_fast", 0)
    for i, (_, snap) in enumerate(refs):
        st.reset_decode_state(d["kv_max"])
        st.load_slot(slots[i], pos[i])
        _same(_snap(st, d, pos[i]), snap)


def test_batch_composition(option_off_afterwards):
    """the 1150-position sequence alone, as row 0 and as row 32 of a 33-row batch of other lengths, and in a permuted batch: the same bits"""
    st, _, d, prompts, firsts, refs = _get(256, 16, False)
    long_i = LENS.index(1150)
    others = [i for i in range(len(LENS)) if i != long_i]
    n_other = 32
    # slots: 0, 1, 2, 3 = the long sequence (one per batch); then three groups of 32 rows cycling through the other sequences
    st.create_slots(4 + 3 * n_other, 1200)
    per_seq = [[] for _ in LENS]
    per_seq[long_i] = [0, 1, 2, 3]
    groups = []
    for g in range(3):
        rows = []
        for r in range(n_other):
            q = others[r % len(others)]; s = 4 + g * n_other + r
            per_seq[q].append(s); rows.append((q, s))
        groups.append(rows)
    _fill_slots(st, d, prompts, per_seq)
    st.set_option("multi_attn_fast", 1)
    want = refs[long_i][0][0]
    batches = [[(long_i, 0)], [(long_i, 1)] + groups[0], groups[1] + [(long_i, 2)]]
    rng = np.random.default_rng(4)
    batches.append([(groups[2] + [(long_i, 3)])[j] for j in rng.permutation(n_other + 1)])
    for rows in batches:
        ids, lg = st.step_multi([s for _, s in rows], [firsts[q] for q, _ in rows], [len(prompts[q]) for q, _ in rows], logits=True)
        for r, (q, _) in enumerate(rows):
            assert np.array_equal(lg[r].view(U), refs[q][0][0][0]), (len(rows), r, LENS[q])
            assert ids[r] == refs[q][0][0][1], (len(rows), r, LENS[q])
        r_long = [q for q, _ in rows].index(long_i)
        assert np.array_equal(lg[r_long].view(U), want[0]), (len(rows), r_long)


@pytest.mark.parametrize("hd,nh,fp8", [(256, 16, False), (128, 8, True)])
def test_within_stated_tolerance_of_the_exact_batched_step(hd, nh, fp8, option_off_afterwards):
    """STATED TOLERANCE (02-numerics.md section 2b, tests/test_attn_fast_gpu.py): max |fast - exact| <= 1e-3 max |exact| on every row's logits,
    same greedy ids; rows of 700 positions or more must differ from the exact bits somewhere (no silent fall-back to the exact kernel)."""
    st, _, d, prompts, firsts, refs = _get(hd, nh, fp8)
    n = len(LENS)
    st.create_slots(2 * n, 1200)
    _fill_slots(st, d, prompts, [[i, n + i] for i in range(n)])
    toks, pos, exact = list(firsts), [len(p) for p in prompts], []
    for k in range(N_STEPS):
        ids, lg = st.step_multi(list(range(n)), toks, pos, logits=True)
        exact.append((toks, ids, lg)); toks = ids; pos = [p + 1 for p in pos]
    st.set_option("multi_attn_fast", 1)
    pos, worst, differs = [len(p) for p in prompts], 0.0, False
    for k, (fed, ids_e, lg_e) in enumerate(exact):
        ids, lg = st.step_multi(list(range(n, 2 * n)), fed, pos, logits=True)
        for i in range(n):
            rel = float(np.abs(lg[i] - lg_e[i]).max() / np.abs(lg_e[i]).max())
            worst = max(worst, rel)
            if LENS[i] >= 700:
                differs |= not np.array_equal(lg[i].view(U), lg_e[i].view(U))
        print(f"hd {hd} fp8 {fp8} step {k}: largest relative error so far {worst:.3e} (bound 1e-3)")
        for i in range(n):
            assert float(np.abs(lg[i] - lg_e[i]).max()) <= 1e-3 * float(np.abs(lg_e[i]).max()), (k, LENS[i])
        assert ids == ids_e, k
        pos = [p + 1 for p in pos]
    assert differs, "no long row differs from the exact step in its bits: the flash-decode did not run"


def test_short_slots_keep_the_exact_step(option_off_afterwards):
    """slots of max_seq <= gqa_split_min: the capacity rule of the store's own fast step -- the exact per-slot kernel, the option-off bits"""
    st, _, d, prompts, firsts, refs = _get(256, 16, False)
    short = [i for i, n in enumerate(LENS) if n < 290]
    n = len(short)
    st.create_slots(2 * n, 300)
    _fill_slots(st, d, [prompts[i] for i in short], [[j, n + j] for j in range(n)])
    runs = []
    for on, base in ((0, 0), (1, n)):
        st.set_option("multi_attn_fast", on)
        toks, pos, out = [firsts[i] for i in short], [LENS[i] for i in short], []
        for _ in range(N_STEPS):
            ids, lg = st.step_multi(list(range(base, base + n)), toks, pos, logits=True)
            out.append((ids, lg.view(U).copy())); toks = ids; pos = [p + 1 for p in pos]
        runs.append(out)
    for (ids0, lg0), (ids1, lg1) in zip(*runs):
        assert ids0 == ids1 and np.array_equal(lg0, lg1)
    st.set_option("multi_attn_fast", 0)
    for j, i in enumerate(short):
        st.reset_decode_state(d["kv_max"]); st.load_slot(j, LENS[i] + N_STEPS); a = _snap(st, d, LENS[i] + N_STEPS)
        st.reset_decode_state(d["kv_max"]); st.load_slot(n + j, LENS[i] + N_STEPS)
        _same(_snap(st, d, LENS[i] + N_STEPS), a)


@pytest.mark.parametrize("sampled", [False, True])
def test_generate_multi_equals_generate_batch_in_fast_mode(sampled, option_off_afterwards):
    st, _, d, prompts, firsts, refs = _get(128, 8, True)
    pick = [LENS.index(n) for n in (1150, 127, 700, 64)]
    P, first = [prompts[i] for i in pick], [firsts[i] for i in pick]
    max_tokens = 6
    params = [(0.6, 50, 0.95, 0.0), (0.9, 7, 0.8, 0.0), (0.0, 0, 1.0, 1.5), (1.2, 0, 0.9, 0.5)] if sampled else [(0.0, 0, 1.0, 0.0)] * 4
    seeds = [0x1234567, 0x9E3779B9, 77, 5]

    def single(i, stop_ids):
        _start(st, d, P[i])
        st.set_attention_mode(True)
        try:
            T, K, TP, PEN = params[i]
            out = st.generate_batch(first[i], len(P[i]), max_tokens, T, K, TP, stop_ids, PEN, rng_seed=seeds[i])
            return out, _snap(st, d, len(P[i]) + len(out))
        finally:
            st.set_attention_mode(False)

    free = [single(i, ())[0] for i in range(4)]
    stop_ids = [free[0][2], free[2][4]]                                     # rows end at different steps; rows without them reach max_tokens
    ref = [single(i, stop_ids) for i in range(4)]
    assert len({len(T) for T, _ in ref}) > 1 and max(len(T) for T, _ in ref) == max_tokens
    slots = [1, 3, 0, 2]
    st.create_slots(4, 1200)
    _fill_slots(st, d, P, [[s] for s in slots])
    st.set_option("multi_attn_fast", 1)
    kw = dict(temperature=[p[0] for p in params], top_k=[p[1] for p in params], top_p=[p[2] for p in params],
              presence_penalty=[p[3] for p in params], rng_seeds=seeds) if sampled else {}
    out = st.generate_multi(slots, first, [len(p) for p in P], max_tokens, stop_ids, **kw)
    assert out == [T for T, _ in ref]
    st.set_option("multi_attn_fast", 0)
    for i in range(4):
        end = len(P[i]) + len(out[i])
        st.reset_decode_state(d["kv_max"])
        st.load_slot(slots[i], end)
        _same(_snap(st, d, end), ref[i][1])


def test_mla_stores_are_refused_under_the_option():
    """an option that silently does nothing on a model family is a trap: with MLA layers every batched entry point raises, naming the option, and
    changes nothing; with the option off again the step is the exact one"""
    import tests.test_multi_mla_gpu as MM
    st, eng, keep, d = MM._build(kv_max=48)
    rng = np.random.default_rng(3)
    prompt = MM._prompt(rng, d, 20)
    ref, _ = MM._reference(st, d, prompt, 2, 1)
    st.create_slots(2, 40)
    MM._fill_slots(st, d, [prompt], [[1]])
    want_slot = MM._snap(st, d, 20)
    st.decode_step(5, 20)                                                   # the store's own logits / last token: must survive the refusals
    want_lg, want_tok = st.read_logits().view(U).copy(), st.last_token()
    st.set_option("multi_attn_fast", 1)
    for call in (lambda: st.step_multi([1], [2], [20]), lambda: st.generate_multi([1], [2], [20], 2), lambda: st.step_multi_sample([1], [2], [20]),
                 lambda: st.generate_multi([1], [2], [20], 2, temperature=0.6, rng_seeds=3)):
        with pytest.raises(Exception, match="multi_attn_fast"):
            call()
        assert np.array_equal(st.read_logits().view(U), want_lg) and st.last_token() == want_tok
    st.set_option("multi_attn_fast", 0)
    st.reset_decode_state(d["kv_max"]); st.load_slot(1, 20)
    MM._same(MM._snap(st, d, 20), want_slot)
    ids, lg = st.step_multi([1], [2], [20], logits=True)
    assert np.array_equal(lg[0].view(U), ref[0][0]) and ids[0] == ref[0][1]


def test_mode_bits_stay_refused_and_the_option_is_isolated(option_off_afterwards):
    st, _, d, prompts, firsts, refs = _get(64, 4, False)
    i = LENS.index(700)
    _start(st, d, prompts[i])
    st.decode_step(firsts[i], 700)                                          # exact single-sequence step: the reference of the option-off step below
    exact_lg, exact_tok = st.read_logits().view(U).copy(), st.last_token()
    st.create_slots(2, 1200)
    _fill_slots(st, d, [prompts[i]], [[0, 1]])
    want = _snap(st, d, 700)
    st.decode_step(9, 700)
    want_lg, want_tok = st.read_logits().view(U).copy(), st.last_token()
    st.set_option("multi_attn_fast", 1)
    for bits in [dict(fast=True), dict(fast=False, gemm_fast=True), dict(fast=False, decode_fast=True)]:
        st.set_attention_mode(**bits)
        for call in (lambda: st.step_multi([0], [2], [700]), lambda: st.generate_multi([0], [2], [700], 2), lambda: st.step_multi_sample([0], [2], [700])):
            with pytest.raises(Exception):
                call()
            assert np.array_equal(st.read_logits().view(U), want_lg) and st.last_token() == want_tok
        st.set_attention_mode(False)
    for s in (0, 1):
        st.reset_decode_state(d["kv_max"]); st.load_slot(s, 700)
        _same(_snap(st, d, 700), want)
    # the option touches the batched steps only: the store's own exact step and prompt pass keep their bits with it set
    _start(st, d, prompts[i])
    st.decode_step(firsts[i], 700)
    assert np.array_equal(st.read_logits().view(U), exact_lg) and st.last_token() == exact_tok
    ids, lg = st.step_multi([0], [firsts[i]], [700], logits=True)           # option on: the single-sequence FAST bits
    assert np.array_equal(lg[0].view(U), refs[i][0][0][0]) and ids[0] == refs[i][0][0][1]
    st.set_option("multi_attn_fast", 0)
    ids, lg = st.step_multi([1], [firsts[i]], [700], logits=True)           # option off again: the exact bits
    assert np.array_equal(lg[0].view(U), exact_lg) and ids[0] == exact_tok
