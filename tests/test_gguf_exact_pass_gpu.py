"""The "gguf_exact_pass" option (docs/design/20-gguf-exact-pass.md): on a store whose MoE layers hold native GGUF blocks, every row of every multi-row
pass -- the batched pass behind the slot entry points, verify, prefill -- carries the bits of kr_decode_step on that sequence alone: logits, greedy id,
KV rows, linear-attention state.  The yardstick everywhere is decode_step, token by token, on the store's own sequence (tests/test_decode_gpu.py holds
it to the oracle's moe_forward_gguf); u32 bit patterns, no tolerances.

Shapes: H 256 (one Q4_K super-block per row) and 512 (two: the block loop runs twice); I 256 (Q4_K down) and 160 (Q8_0 down, 5 blocks: a ragged last
group of 4); H 2304 (a second, partial k stage of the grouped kernels); E 8 / top 3 at 40 rows (~15 rows per expert: several groups of 8, the last one partial); E 16 / top 4 at one row (experts with 0 or 1 rows)."""
import numpy as np
import pytest

from oracle import oracle as O
from tests.test_decode_gpu import build
from tests.test_speculative_gpu import _same, _snap
from tests.test_multi_extend_gpu import _assert_rows, _reference, _slot_state, _toks
from tests.test_multi_verify_gpu import _check_slot, _right, _trace, _wrong_at
from tests import test_multi_mla_gpu as mla

pytestmark = pytest.mark.gpu
F = np.float32
U = np.uint32

KV = 64
# name -> (builder kind, dims (H, V, E, k, I, SI), gate|up / down types or True = Q4_K with Q4_K / Q8_0 down by I)
STORES = {
    "hybrid-q4k-q4k": ("hybrid", (256, 512, 8, 3, 256, 128), True),
    "hybrid-h512-q4k-q8_0": ("hybrid", (512, 512, 8, 3, 160, 128), True),
    "mla-q4k-q4k": ("mla", (256, 384, 8, 3, 256, 256), True),
    "mla-q4k-q8_0": ("mla", (256, 384, 8, 3, 160, 256), True),
    "hybrid-e16-k4": ("hybrid", (256, 512, 16, 4, 128, 128), True),
    "hybrid-q4_0-gate": ("hybrid", (256, 512, 8, 3, 256, 128), (O.Q4_0, O.Q4_K)),      # a fallback type: gate | up Q4_0 has no grouped form
    "hybrid-rsf2.5-sigmoid": ("hybrid", (256, 512, 8, 3, 256, 128), True),             # rsf != 1: the store's factor in the epilogue, nowhere else
}
STORES.update({      # K = 2304 = 9 super-blocks / 72 blocks: the kernels' second k stage (a stage is 2048 k), partial
    "hybrid-h2304-q4k": ("hybrid", (2304, 512, 8, 3, 256, 128), True),
    "hybrid-h2304-q8_0": ("hybrid", (2304, 512, 8, 3, 256, 128), (O.Q8_0, O.Q8_0)),
})
EXTRA = {"hybrid-rsf2.5-sigmoid": dict(norm_bias_one=False, scoring=0, rsf=2.5)}


def _store(name, option=True, kv_max=KV):
    kind, dims, types = STORES[name]
    if kind == "mla":
        st, eng, keep, d = mla._build(kv_max=kv_max, gguf=True, dims=dims)
        snap, same = mla._snap, mla._same
    else:
        st, eng, orc, keep, d = build(kv_max=kv_max, dims=dims, gguf=types, seed=11, **EXTRA.get(name, {}))
        snap, same = _snap, _same
    if option:
        st.set_option("gguf_exact_pass", 1)
    d["_keep"] = (eng, keep)
    return st, d, snap, same


def _rows(st, d, snap, n_seq, groups, seed=5):
    """n_seq sequences (prompts of 0..5 tokens by decode_step, then one token): references, and the sequences saved into the slots of `groups` =
    [(sequence indices, first slot)]"""
    rng = np.random.default_rng(seed)
    prompts = [_toks(rng, d, int(rng.integers(0, 6))) for _ in range(n_seq)]
    firsts = _toks(rng, d, n_seq)
    fills = [[] for _ in range(n_seq)]
    for seqs, base in groups:
        for r, q in enumerate(seqs):
            fills[q].append(base + r)
    refs = [_reference(st, d, p, [f], fill, snap=snap) for p, f, fill in zip(prompts, firsts, fills)]
    return prompts, firsts, refs


def _fill(st, d, prompt, slots):
    """the prompt by decode_step from zero state, saved into `slots`; the store stays at the prompt's end"""
    st.reset_decode_state(d["kv_max"])
    for i, t in enumerate(prompt):
        st.decode_step(t, i)
    for s in slots:
        st.save_slot(s, len(prompt))


def _step_group(st, seqs, base, prompts, firsts):
    slots = list(range(base, base + len(seqs)))
    return slots, st.step_multi(slots, [firsts[q] for q in seqs], [len(prompts[q]) for q in seqs], logits=True)


def _assert_group(st, seqs, slots, refs, ids, lg, follow=True, between=None):
    for r, q in enumerate(seqs):
        assert np.array_equal(lg[r].view(U), refs[q]["lg"]), ("logits", len(seqs), r, q)
        assert ids[r] == refs[q]["tok"], ("id", len(seqs), r, q)
    if between:
        between()
    if follow:      # the following step: the slots continue as the sequences do
        ids2, lg2 = st.step_multi(slots, ids, [refs[q]["pos"] for q in seqs], logits=True)
        for r, q in enumerate(seqs):
            assert np.array_equal(lg2[r].view(U), refs[q]["next"][0]) and ids2[r] == refs[q]["next"][1], ("next", len(seqs), r, q)


@pytest.mark.parametrize("name", ["hybrid-q4k-q4k", "hybrid-h512-q4k-q8_0", "mla-q4k-q4k", "mla-q4k-q8_0", "hybrid-rsf2.5-sigmoid", "hybrid-h2304-q4k", "hybrid-h2304-q8_0"])
def test_step_multi_rows_of_1_5_40_equal_decode_step(name):
    st, d, snap, same = _store(name)
    st.create_slots(46, 16)
    perm = [int(x) for x in np.random.default_rng(3).permutation(40)]
    groups = [([7], 0), ([30, 2, 11, 25, 4], 1), (perm, 6)]                  # slots and rows not in sequence order
    prompts, firsts, refs = _rows(st, d, snap, 40, groups)

    def states():                                                           # the KV rows / states the step left in the slots of the 5-row group
        for r, q in enumerate(groups[1][0]):
            same(_slot_state(st, d, 1 + r, refs[q]["pos"], snap), refs[q]["snap"])

    for seqs, base in groups:
        slots, (ids, lg) = _step_group(st, seqs, base, prompts, firsts)
        _assert_group(st, seqs, slots, refs, ids, lg, between=states if len(seqs) == 5 else None)


@pytest.mark.parametrize("name", ["hybrid-q4k-q4k", "mla-q4k-q8_0"])
def test_generate_multi_equals_generate_batch(name):
    st, d, snap, same = _store(name)
    st.create_slots(5, 32)
    rng = np.random.default_rng(13)
    prompts, firsts, n_tok = [_toks(rng, d, n) for n in (5, 0, 9, 2, 3)], _toks(rng, d, 5), 6
    slots, want = [3, 0, 4, 2, 1], []
    for p, f, s in zip(prompts, firsts, slots):
        _fill(st, d, p, [s])
        T = st.generate_batch(f, len(p), n_tok)
        want.append((T, snap(st, d, len(p) + n_tok)))
    got = st.generate_multi(slots, firsts, [len(p) for p in prompts], n_tok)
    assert got == [w[0] for w in want]
    for s, p, w in zip(slots, prompts, want):
        same(_slot_state(st, d, s, len(p) + n_tok, snap), w[1])


def test_one_row_with_16_experts_top_4():
    st, d, snap, same = _store("hybrid-e16-k4")
    st.create_slots(1, 16)
    prompts, firsts, refs = _rows(st, d, snap, 1, [([0], 0)])
    slots, (ids, lg) = _step_group(st, [0], 0, prompts, firsts)
    _assert_group(st, [0], slots, refs, ids, lg)


@pytest.mark.parametrize("name", ["hybrid-q4k-q4k", "hybrid-h512-q4k-q8_0", "mla-q4k-q4k"])
def test_extend_multi_equals_decode_steps_and_is_cut_invariant(name):
    st, d, snap, same = _store(name)
    st.create_slots(8, 40)
    rng = np.random.default_rng(5)
    seqs, slots = [(0, 1), (3, 9), (7, 16), (2, 3)], [3, 0, 6, 2]              # runs of 1, 9, 16 and 3 tokens in one call
    prompts = [_toks(rng, d, p) for p, _ in seqs]
    runs = [_toks(rng, d, r) for _, r in seqs]
    refs = [_reference(st, d, p, r, [s] + ([7] if len(r) == 9 else []), snap=snap) for p, r, s in zip(prompts, runs, slots)]
    ids, lg = st.extend_multi(slots, runs, [len(p) for p in prompts], logits=True)
    _assert_rows(st, d, refs, slots, ids, lg, same=same, snap=snap)
    st.extend_multi([7], [runs[1][:4]], [3])                                   # extend 9 = extend 4 + extend 5
    ids2, lg2 = st.extend_multi([7], [runs[1][4:]], [7], logits=True)
    _assert_rows(st, d, [refs[1]], [7], ids2, lg2, same=same, snap=snap)


def test_rows_do_not_depend_on_their_group():
    """a row of a 40-row pass has the bits of that row passed alone, and of the same row in another permutation of the pass"""
    st, d, snap, same = _store("hybrid-q4k-q4k")
    st.create_slots(86, 16)
    rng = np.random.default_rng(17)
    p1, p2, few = [int(x) for x in rng.permutation(40)], [int(x) for x in rng.permutation(40)], [0, 13, 21, 39, 8, 30]
    groups = [(p1, 0), (p2, 40)] + [([q], 80 + i) for i, q in enumerate(few)]
    prompts, firsts, refs = _rows(st, d, snap, 40, groups, seed=19)
    _, (ids1, lg1) = _step_group(st, p1, 0, prompts, firsts)
    _, (ids2, lg2) = _step_group(st, p2, 40, prompts, firsts)
    for r, q in enumerate(p1):
        r2 = p2.index(q)
        assert np.array_equal(lg1[r].view(U), lg2[r2].view(U)) and ids1[r] == ids2[r2], ("permutation", q)
    for i, q in enumerate(few):
        _, (ids, lg) = _step_group(st, [q], 80 + i, prompts, firsts)
        r = p1.index(q)
        assert np.array_equal(lg[0].view(U), lg1[r].view(U)) and ids[0] == ids1[r], ("alone", q)
        same(_slot_state(st, d, 80 + i, refs[q]["pos"], snap), _slot_state(st, d, r, refs[q]["pos"], snap))


@pytest.mark.parametrize("name", ["hybrid-q4k-q4k", "mla-q4k-q8_0"])
def test_verify_multi_and_commit_multi(name):
    """all drafts right, the first wrong draft at another index per row, one row that keeps nothing"""
    st, d, snap, same = _store(name)
    st.create_slots(8, 60)
    rng = np.random.default_rng(7)
    js, slots, pre, c = [None, 2, 5, 7], [4, 1, 7, 0, 3], [3, 0, 11, 6, 2], 9
    trs = [_trace(st, d, _toks(rng, d, p), _toks(rng, d, 1)[0], 12, [s], snap) for p, s in zip(pre, slots)]
    runs = [_right(tr, c) if j is None else _wrong_at(tr, c, j, d["V"]) for tr, j in zip(trs, js)] + [_right(trs[4], c)]
    pos = [tr["p0"] for tr in trs]
    greedy, nm = st.verify_multi(slots, runs, pos)
    keeps = []
    for i, j in enumerate(js):
        n = c if j is None else j
        assert nm[i] == n - 1, (i, nm)
        assert greedy[i][:n] == trs[i]["toks"][1:n + 1], i
        keeps.append(n)
    st.commit_multi(keeps + [0])
    for tr, n, s in zip(trs, keeps, slots):
        _check_slot(st, d, s, tr, n, snap, same)
    _check_slot(st, d, slots[4], trs[4], 0, snap, same)                       # n_keep = 0: as before the verify
    ids, lg = st.step_multi(slots[:4], [tr["toks"][n] for tr, n in zip(trs, keeps)], [p + n for p, n in zip(pos, keeps)], logits=True)
    for i, (tr, n) in enumerate(zip(trs, keeps)):
        assert np.array_equal(lg[i].view(U), tr["lg"][n]) and ids[i] == tr["toks"][n + 1], i


def test_generate_multi_lookup_forms_equal_generate_multi():
    from tests.test_multi_verify_sample_gpu import _lookup_equals_generate
    st, d, snap, same = _store("hybrid-q4k-q4k")
    st.create_slots(10, 60)
    rng = np.random.default_rng(23)
    prompts, firsts, n_tok = [_toks(rng, d, p) for p in (5, 0, 9)], _toks(rng, d, 3), 10
    A, B = [6, 1, 4], [0, 7, 2]
    for p, a, b in zip(prompts, A, B):
        _fill(st, d, p, [a, b])
    pos = [len(p) for p in prompts]
    want = st.generate_multi(B, firsts, pos, n_tok)
    got = st.generate_multi_lookup(A, firsts, pos, n_tok, contexts=[[f] + w for f, w in zip(firsts, want)], max_draft=4)
    assert got == want
    assert st.last_multi_lookup_stats["passes"] < n_tok
    for a, b, p, w in zip(A, B, pos, want):
        _same(_slot_state(st, d, a, p + len(w)), _slot_state(st, d, b, p + len(w)))

    def speculated(stats, n):
        assert stats["passes"] < n, stats

    _lookup_equals_generate(st, d, 4, 4, ((True, False), (False, False)), speculated)      # the sampled loop: tokens, slot state, sampler state


@pytest.mark.parametrize("name", ["hybrid-q4k-q4k", "hybrid-h512-q4k-q8_0", "mla-q4k-q4k"])
def test_single_sequence_prefill_verify_and_lookup(name):
    st, d, snap, same = _store(name)
    rng = np.random.default_rng(29)
    toks = _toks(rng, d, 34)
    st.reset_decode_state(d["kv_max"])
    for i, t in enumerate(toks):
        st.decode_step(t, i)
    want = (st.read_logits().view(U).copy(), st.last_token(), snap(st, d, 34))
    st.reset_decode_state(d["kv_max"])
    st.set_prefill_chunk(12)                                                   # three chunks in flight
    st.prefill(toks[:33], 0)
    st.decode_step(toks[33], 33)
    assert np.array_equal(st.read_logits().view(U), want[0]) and st.last_token() == want[1]
    same(snap(st, d, 34), want[2])
    first, start, n = 5, 3, 12
    st.reset_decode_state(d["kv_max"])
    st.prefill(toks[:start], 0)
    T = st.generate_batch(first, start, n)
    ref = (st.read_logits().view(U).copy(), snap(st, d, start + n))
    st.reset_decode_state(d["kv_max"])
    st.prefill(toks[:start], 0)
    greedy, m = st.verify([first] + T[:5], start)
    assert greedy == T[:6] and m == 5
    st.commit(2)
    assert st.generate_batch(T[1], start + 2, n - 2) == T[2:]
    st.reset_decode_state(d["kv_max"])
    st.prefill(toks[:start], 0)
    assert st.generate_lookup(first, start, n, context=[first] + T, max_draft=4) == T
    assert np.array_equal(st.read_logits().view(U), ref[0])
    same(snap(st, d, start + n), ref[1])


@pytest.mark.parametrize("name", ["hybrid-q4k-q4k", "hybrid-h512-q4k-q8_0", "hybrid-q4_0-gate"])
def test_streaming_hook_and_fallback_types_give_decode_bits(name):
    """ "gguf_exact_grouped" 0 (the streaming kernels for every type) and a layer of a type without a grouped form: decode's bits either way"""
    st, d, snap, same = _store(name)
    st.create_slots(80, 16)
    perm = [int(x) for x in np.random.default_rng(3).permutation(40)]
    groups = [(perm, 0), (perm, 40)]
    prompts, firsts, refs = _rows(st, d, snap, 40, groups)
    got = []
    for grouped, base in ((1, 0), (0, 40)):
        st.set_option("gguf_exact_grouped", grouped)
        slots, (ids, lg) = _step_group(st, perm, base, prompts, firsts)
        _assert_group(st, perm, slots, refs, ids, lg, follow=False)
        got.append((ids, lg.view(U).copy()))
    st.set_option("gguf_exact_grouped", 1)
    assert got[0][0] == got[1][0] and np.array_equal(got[0][1], got[1][1])


def test_refusals():
    st, d, snap, same = _store("hybrid-q4k-q4k", option=False)
    st.create_slots(3, 24)
    st.reset_decode_state(d["kv_max"])
    for t in range(4):
        st.decode_step(t + 1, t)
    own = lambda: (st.read_logits().view(U).copy(), st.last_token(), snap(st, d, 4))
    want = own()

    def unchanged():
        got = own()
        assert np.array_equal(got[0], want[0]) and got[1] == want[1]
        same(got[2], want[2])

    for call in (lambda: st.step_multi([0], [1], [0]), lambda: st.save_slot(0, 4), lambda: st.verify([1, 2], 4)):      # option off: the GGUF refusal, with the hint
        with pytest.raises(RuntimeError, match="GGUF.*gguf_exact_pass"):
            call()
    unchanged()
    st.set_option("gguf_exact_pass", 1)
    st.save_slot(1, 4)
    for mode in (dict(fast=True), dict(fast=False, gemm_fast=True), dict(fast=False, decode_fast=True)):               # option on: every tolerance bit still refuses
        st.set_attention_mode(**mode)
        for call in (lambda: st.step_multi([1], [2], [4]), lambda: st.verify([1, 2], 4), lambda: st.extend_multi([1], [[2, 3]], [4])):
            with pytest.raises(RuntimeError, match="exact-mode only"):
                call()
    st.set_attention_mode(False, gemm_fast=True)
    for call in (lambda: st.prefill([1, 2, 3], 4), lambda: st.prefill_nll([1, 2, 3], 4)):                               # option + KR_GEMM_FAST: no prompt pass
        with pytest.raises(RuntimeError, match="gguf_exact_pass.*KR_GEMM_FAST"):
            call()
    st.set_attention_mode(False)
    unchanged()
    same(_slot_state(st, d, 1, 4, snap), want[2])                              # the slot too (this resets the store: last)


def test_option_on_a_store_without_gguf_layers_changes_nothing():
    st, eng, orc, keep, d = build(kv_max=KV, dims=(256, 512, 8, 3, 256, 128), seed=11)
    st.create_slots(10, 16)
    prompts, firsts, refs = _rows(st, d, _snap, 5, [(list(range(5)), 0), (list(range(5)), 5)])
    slots, (ids, lg) = _step_group(st, list(range(5)), 0, prompts, firsts)
    st.set_option("gguf_exact_pass", 1)
    slots2, (ids2, lg2) = _step_group(st, list(range(5)), 5, prompts, firsts)
    assert ids == ids2 and np.array_equal(lg.view(U), lg2.view(U))
    _assert_group(st, list(range(5)), slots2, refs, ids2, lg2)
    st.set_attention_mode(False, gemm_fast=True)                                # no GGUF layer: the tolerance prompt pass keeps running under the option
    st.reset_decode_state(d["kv_max"])
    st.prefill([1, 2, 3], 0)
    st.set_attention_mode(False)
