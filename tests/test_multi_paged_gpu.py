"""Paged sequence slots (kr_decode_slots_create_paged / kr_decode_slot_trim / kr_decode_slots_pages; docs/design/21-paged-slots.md): a paged slot set
behaves as a flat one of the same n_slots and max_seq through every slot entry point, bit for bit -- ids, logits, n_match, stored rows, conv and recurrent
state, sampler state -- while the GQA / MLA rows live in pages shared by all slots.  The reference is the single-sequence path (decode_step,
generate_batch, prefill + state read-back), which the existing suites hold to the CPU oracle; where a whole call sequence is compared, the same sequence
also runs on flat slots of the same store.  The paged path is never compared with itself.  Every assertion is on ids and u32 / stored-row bit patterns."""
import numpy as np
import pytest

from krasis_amd._lib import KrasisHipError
from tests import test_multi_mla_gpu as mla
from tests import test_multi_seq_gpu as seq
from tests.test_decode_gpu import build
from tests.test_speculative_gpu import _same, _snap

pytestmark = pytest.mark.gpu
U = np.uint32
PT = 32


class Gqa:
    """the hybrid linear-attention + GQA test model and its single-sequence reference helpers"""
    reference = staticmethod(seq._reference)
    start = staticmethod(seq._start)
    snap = staticmethod(_snap)
    same = staticmethod(_same)

    @staticmethod
    def build(fp8=False, **kw):
        st, eng, orc, keep, d = build(**kw)
        if fp8:
            st.set_kv_dtype(True); d["fp8"] = True
        return st, (eng, orc, keep), d


class Mla:
    reference = staticmethod(mla._reference)
    start = staticmethod(mla._start)
    snap = staticmethod(mla._snap)
    same = staticmethod(mla._same)

    @staticmethod
    def build(fp8=False, **kw):
        st, eng, keep, d = mla._build(fp8, **kw)
        return st, (eng, keep), d


def _toks(rng, d, n):
    return [int(x) for x in rng.integers(0, d["V"], n)]


def _pages(n):
    return (n + PT - 1) // PT


def _slot_state(K, st, d, slot, pos):
    st.reset_decode_state(d["kv_max"])
    st.load_slot(slot, pos)
    return K.snap(st, d, pos)


def _state_error(call, *needles):
    """the call is refused with KR_ERR_STATE (RuntimeError, not a HIP failure) and its message names every needle"""
    with pytest.raises(RuntimeError) as e:
        call()
    assert not isinstance(e.value, KrasisHipError), e.value
    for s in needles:
        assert s in str(e.value), (s, str(e.value))


# ---- 1, 2: prompts enter by prefill_slot in chunks that straddle page edges, then 40 steps cross positions 32, 64 and 96 at different steps ---------------
def _prefill_then_steps(K, st, d, n_pages, page_tokens=PT, lens=(0, 31, 70), n_steps=40, max_seq=120):
    rng = np.random.default_rng(11)
    prompts = [_toks(rng, d, n) for n in lens]
    firsts = _toks(rng, d, len(lens))
    refs = [K.reference(st, d, p, f, n_steps) for p, f in zip(prompts, firsts)]
    st.create_slots(len(lens) + 1, max_seq, page_tokens=page_tokens, n_pages=n_pages)
    slots = [2, 0, 3][:len(lens)]
    for s, p in zip(slots, prompts):
        if p:
            st.prefill_slot(s, p, chunk=24)
    pages = st.slot_pages()
    assert pages["page_tokens"] == page_tokens and pages["n_pages"] == n_pages
    assert [pages["per_slot"][s] for s in slots] == [(len(p) + page_tokens - 1) // page_tokens for p in prompts]
    toks, pos = list(firsts), [len(p) for p in prompts]
    for k in range(n_steps):
        ids, lg = st.step_multi(slots, toks, pos, logits=True)
        for i, (ref, _) in enumerate(refs):
            assert np.array_equal(lg[i].view(U), ref[k][0]), ("logits", k, i)
            assert ids[i] == ref[k][1], ("id", k, i)
        toks = ids; pos = [p + 1 for p in pos]
    pages = st.slot_pages()
    assert [pages["per_slot"][s] for s in slots] == [(p + page_tokens - 1) // page_tokens for p in pos]
    assert pages["free"] == n_pages - sum(pages["per_slot"])
    for i, (_, snap) in enumerate(refs):
        K.same(_slot_state(K, st, d, slots[i], pos[i]), snap)


@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("hd,nh", [(64, 4), (128, 8), (256, 16)])
def test_hybrid_prefill_and_steps_equal_decode_step_alone(hd, nh, fp8):
    st, keep, d = Gqa.build(fp8, seed=3, hd=hd, nh=nh, kv_max=128)
    _prefill_then_steps(Gqa, st, d, n_pages=10)


@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("cfg", mla.CFGS)
def test_mla_prefill_and_steps_equal_decode_step_alone(cfg, fp8):
    st, keep, d = Mla.build(fp8, kv_max=128, **cfg)
    _prefill_then_steps(Mla, st, d, n_pages=10)


# ---- 3: scattered, reused and dirty pages ---------------------------------------------------------------------------------------------------------------
def _scattered(K, st, d, paged, seqs, probe):
    """the call sequence of test 3 on paged or flat slots -> everything it produced"""
    (pa, fa), (pb, fb), (pc, _) = seqs
    st.create_slots(4, 120, **(dict(page_tokens=PT, n_pages=8) if paged else {}))
    out = []
    out.append(st.extend_multi([0], [pa[:20]], [0]))          # slot 0: page 0
    out.append(st.extend_multi([1], [pb], [0]))               # slot 1: page 1
    out.append(st.extend_multi([2], [pc], [0]))               # slot 2: pages 2, 3
    out.append(st.extend_multi([0], [pa[20:]], [20]))         # slot 0 grows over position 32: page 4, its ids are now [0, 4]
    if paged:
        assert st.slot_pages()["per_slot"] == [2, 1, 2, 0] and st.slot_pages()["free"] == 3
    st.trim_slot(2, 0)                                         # pages 2 and 3 go back, holding sequence c's rows
    if paged:
        assert st.slot_pages()["per_slot"] == [2, 1, 0, 0] and st.slot_pages()["free"] == 5
    toks, pos, steps = [fa, fb], [len(pa), len(pb)], []
    for k in range(35):                                        # slot 1 takes dirty page 2 at position 32, slot 0 dirty page 3 at position 64: ids [0, 4, 3]
        ids, lg = st.step_multi([0, 1], toks, pos, logits=True)
        steps.append((lg.view(U).copy(), list(ids)))
        toks = ids; pos = [p + 1 for p in pos]
    if paged:
        assert st.slot_pages()["per_slot"] == [_pages(pos[0]), _pages(pos[1]), 0, 0]
    states = [_slot_state(K, st, d, 0, pos[0]), _slot_state(K, st, d, 1, pos[1])]
    st.trim_slot(1, 0)                                         # pages 1 and 2 go back, holding sequence b's rows
    ids, lg = st.step_multi([3], [probe], [40], logits=True)   # a never-filled slot at position 40 maps them: they must read as zero
    if paged:
        assert st.slot_pages()["per_slot"] == [_pages(pos[0]), 0, 0, 2]
    return out, steps, states, (lg.view(U).copy(), list(ids))


@pytest.mark.parametrize("K,fp8", [(Gqa, False), (Gqa, True), (Mla, False), (Mla, True)])
def test_scattered_and_reused_pages(K, fp8):
    st, keep, d = K.build(fp8, kv_max=128)
    rng = np.random.default_rng(21)
    seqs = [(_toks(rng, d, n), _toks(rng, d, 1)[0]) for n in (33, 20, 40)]
    probe = _toks(rng, d, 1)[0]
    refs = [K.reference(st, d, p, f, 35) for p, f in seqs[:2]]
    got = _scattered(K, st, d, True, seqs, probe)
    flat = _scattered(K, st, d, False, seqs, probe)
    for k, (lg, ids) in enumerate(got[1]):
        for i, (ref, _) in enumerate(refs):
            assert np.array_equal(lg[i], ref[k][0]) and ids[i] == ref[k][1], (k, i)
    for i, (_, snap) in enumerate(refs):
        K.same(got[2][i], snap)
    assert got[0] == flat[0]
    for (lg, ids), (flg, fids) in zip(got[1], flat[1]):
        assert np.array_equal(lg, flg) and ids == fids
    assert np.array_equal(got[3][0], flat[3][0]) and got[3][1] == flat[3][1]      # the probe step: what a fresh flat slot gives


# ---- 4: a pool smaller than n_slots x max_seq -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [Gqa, Mla])
def test_small_pool_refuses_the_ninth_page(K):
    st, keep, d = K.build(kv_max=160)
    rng = np.random.default_rng(31)
    lens = (60, 40, 33, 20)                                    # 2 + 2 + 2 + 1 pages
    prompts = [_toks(rng, d, n) for n in lens]
    firsts = _toks(rng, d, 4)
    refs = [K.reference(st, d, p, f, 6) for p, f in zip(prompts, firsts)]
    st.create_slots(4, 160, page_tokens=PT, n_pages=8)
    slots = [0, 1, 2, 3]
    for s, p in zip(slots, prompts):
        st.prefill_slot(s, p, chunk=24)
    toks, pos = list(firsts), list(lens)
    for k in range(5):                                         # slot 0 reaches position 64 in the fifth step: the eighth page
        ids, lg = st.step_multi(slots, toks, pos, logits=True)
        for i, (ref, _) in enumerate(refs):
            assert np.array_equal(lg[i].view(U), ref[k][0]) and ids[i] == ref[k][1], (k, i)
        toks = ids; pos = [p + 1 for p in pos]
    before = st.slot_pages()
    assert before["per_slot"] == [3, 2, 2, 1] and before["free"] == 0
    # slot 3 from position 25 over position 32 needs a ninth page: row 1 of the call
    _state_error(lambda: st.extend_multi([0, 3], [[toks[0]], [toks[3]] + _toks(rng, d, 7)], [pos[0], pos[3]]), "row 1", "slot 3")
    _state_error(lambda: st.generate_multi([0, 3], [toks[0], toks[3]], [pos[0], pos[3]], 8), "row 1")
    _state_error(lambda: st.verify_multi([3], [[toks[3]] + _toks(rng, d, 7)], [pos[3]]), "row 0")
    assert st.slot_pages() == before
    ids, lg = st.step_multi(slots, toks, pos, logits=True)    # the next legal step
    for i, (ref, _) in enumerate(refs):
        assert np.array_equal(lg[i].view(U), ref[5][0]) and ids[i] == ref[5][1], i
    pos = [p + 1 for p in pos]
    for i, (_, snap) in enumerate(refs):
        K.same(_slot_state(K, st, d, slots[i], pos[i]), snap)
    # save_slot: the store's own sequence of 40 positions into slot 3 needs a second page there
    K.start(st, d, prompts[1])
    want = K.snap(st, d, 40)
    _state_error(lambda: st.save_slot(3, 40), "slot 3")
    assert st.slot_pages() == before
    K.same(K.snap(st, d, 40), want)
    st.trim_slot(2, 0)
    st.save_slot(3, 40)
    assert st.slot_pages()["per_slot"] == [3, 2, 0, 2]
    K.same(_slot_state(K, st, d, 3, 40), want)
    K.same(_slot_state(K, st, d, 0, pos[0]), refs[0][1])      # the other slots are where they were


# ---- 5: speculation ------------------------------------------------------------------------------------------------------------------------------------
SPEC_LENS = (28, 60, 5)                                        # runs of 8 from 28 and 60 straddle positions 32 and 64
SAMPLER = dict(temperature=[0.0, 0.8, 1.0], top_k=[0, 20, 0], top_p=[1.0, 0.9, 1.0], presence_penalty=[1.5, 0.0, 0.5], rng_seeds=[7, 8, 9])


def _speculation(K, st, d, paged, prompts, runs):
    new = lambda: st.create_slots(4, 120, **(dict(page_tokens=PT, n_pages=12) if paged else {}))
    slots, out = [2, 0, 3], []
    fill = lambda: [st.prefill_slot(s, p, chunk=24) for s, p in zip(slots, prompts)]
    for keep_of in (lambda m: 0, lambda m: 1, lambda m: m + 1):
        for sample in (False, True):
            new(); fill()
            if sample:
                for i, s in enumerate(slots):
                    st.set_slot_sampler(s, runs[i][0], SAMPLER["temperature"][i], SAMPLER["top_k"][i], SAMPLER["top_p"][i], SAMPLER["presence_penalty"][i], SAMPLER["rng_seeds"][i])
            ids, nm = (st.verify_multi_sample if sample else st.verify_multi)(slots, runs, list(SPEC_LENS))
            if paged:                                          # the drafted positions are mapped, and stay mapped over the commit
                assert [st.slot_pages()["per_slot"][s] for s in slots] == [_pages(n + 8) for n in SPEC_LENS]
                with pytest.raises(RuntimeError):
                    st.trim_slot(0, 0)                         # refused while the verify is pending
            keep = [keep_of(m) for m in nm]
            st.commit_multi(keep)
            if paged:
                assert [st.slot_pages()["per_slot"][s] for s in slots] == [_pages(n + 8) for n in SPEC_LENS]
            out.append(([g[:m + 1] for g, m in zip(ids, nm)], nm, [_slot_state(K, st, d, s, n + k) for s, n, k in zip(slots, SPEC_LENS, keep)],
                        [st.slot_sampler_state(s) for s in slots]))
    for sampler in (None, SAMPLER):
        new(); fill()
        firsts, ctx = [r[0] for r in runs], [p + p for p in prompts]
        if sampler:
            T = st.generate_multi_lookup_sample(slots, firsts, list(SPEC_LENS), 14, ctx, 7, 2, **sampler)
        else:
            T = st.generate_multi_lookup(slots, firsts, list(SPEC_LENS), 14, ctx, 7, 2)
        if paged:
            assert [st.slot_pages()["per_slot"][s] for s in slots] == [_pages(n + len(t)) for n, t in zip(SPEC_LENS, T)]
        out.append((T, dict(st.last_multi_lookup_stats), [_slot_state(K, st, d, s, n + len(t)) for s, n, t in zip(slots, SPEC_LENS, T)],
                    [st.slot_sampler_state(s) for s in slots]))
    return out


def _equal_runs(K, got, flat):
    assert len(got) == len(flat)
    for (a, b, states, smp), (fa, fb, fstates, fsmp) in zip(got, flat):
        assert a == fa and b == fb
        for x, y in zip(states, fstates):
            K.same(x, y)
        for (seen, rng), (fseen, frng) in zip(smp, fsmp):
            assert np.array_equal(seen, fseen) and rng == frng


@pytest.mark.parametrize("K", [Gqa, Mla])
def test_speculation_equals_the_flat_run(K):
    st, keep, d = K.build(kv_max=128)
    rng = np.random.default_rng(41)
    prompts = [_toks(rng, d, n) for n in SPEC_LENS]
    firsts = _toks(rng, d, 3)
    truth = []
    for p, f in zip(prompts, firsts):                          # the single-sequence continuation: what an all-right draft is
        K.start(st, d, p); truth.append(st.generate_batch(f, len(p), 14))
    runs = [[f] + t[:7] for f, t in zip(firsts, truth)]
    runs[2][3] = (runs[2][3] + 1) % d["V"]                     # row 2: a wrong draft at index 3
    got = _speculation(K, st, d, True, prompts, runs)
    flat = _speculation(K, st, d, False, prompts, runs)
    _equal_runs(K, got, flat)
    for r in (0, 2, 4):                                        # the greedy verifies against the reference: ids after every token, n_match
        ids, nm = got[r][0], got[r][1]
        assert nm == [7, 7, 2]
        assert ids[0] == truth[0][:8] and ids[1] == truth[1][:8] and ids[2] == truth[2][:3]
    assert got[6][0] == truth                                  # generate_multi_lookup = generate_batch on each sequence alone


# ---- 6: generate ---------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [Gqa, Mla])
def test_generate_gives_back_what_it_mapped(K):
    st, keep, d = K.build(kv_max=160)
    rng = np.random.default_rng(51)
    lens, max_tokens = (30, 50, 3), 60
    prompts = [_toks(rng, d, n) for n in lens]
    firsts = _toks(rng, d, 3)
    free_run = []
    for p, f in zip(prompts, firsts):
        K.start(st, d, p); free_run.append(st.generate_batch(f, len(p), max_tokens))
    stop = [free_run[0][4], free_run[2][9]]                    # rows 0 and 2 stop early
    ref, snaps = [], []
    for p, f in zip(prompts, firsts):
        K.start(st, d, p); T = st.generate_batch(f, len(p), max_tokens, stop_ids=stop)
        ref.append(T); snaps.append(K.snap(st, d, len(p) + len(T)))
    assert len(ref[0]) < 20 and len(ref[2]) < 20
    outs = []
    for paged in (True, False):
        st.create_slots(3, 160, **(dict(page_tokens=PT, n_pages=15) if paged else {}))
        for s, p in enumerate(prompts):
            st.prefill_slot(s, p, chunk=24)
        st.verify_multi([2], [[1]], [100]); st.commit_multi([0])      # slot 2 holds pages 0 .. 3 from before the call, past anything it will generate
        if paged:
            assert st.slot_pages()["per_slot"] == [1, 2, 4]
        T = st.generate_multi([0, 1, 2], firsts, list(lens), max_tokens, stop)
        assert T == ref
        final = [n + len(t) for n, t in zip(lens, T)]
        if paged:
            pages = st.slot_pages()
            assert pages["per_slot"] == [_pages(final[0]), _pages(final[1]), 4], pages
            assert pages["free"] == 15 - sum(pages["per_slot"])
        for s in range(3):
            K.same(_slot_state(K, st, d, s, final[s]), snaps[s])
        outs.append(T)
    assert outs[0] == outs[1]


# ---- 7: save / load ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,fp8", [(Gqa, False), (Gqa, True), (Mla, False), (Mla, True)])
def test_save_load_round_trip(K, fp8):
    st, keep, d = K.build(fp8, kv_max=128)
    rng = np.random.default_rng(61)
    prompt = _toks(rng, d, 95)
    K.start(st, d, prompt)
    want = {n: K.snap(st, d, n) for n in (33, 95)}
    st.create_slots(2, 100, page_tokens=PT, n_pages=5)
    st.save_slot(1, 33)
    assert st.slot_pages()["per_slot"] == [0, 2]
    K.same(_slot_state(K, st, d, 1, 33), want[33])
    K.start(st, d, prompt)
    st.save_slot(0, 95)
    assert st.slot_pages()["per_slot"] == [3, 2] and st.slot_pages()["free"] == 0
    K.same(_slot_state(K, st, d, 0, 95), want[95])
    K.same(_slot_state(K, st, d, 1, 33), want[33])
    st.trim_slot(0, 40)                                        # page 2 (positions 64 ..) is gone: its rows load as zero, the others as saved
    assert st.slot_pages()["per_slot"] == [2, 2]
    K.start(st, d, prompt)                                     # the store's rows are non-zero before the load
    st.load_slot(0, 95)
    got = K.snap(st, d, 95)
    parts = lambda layer: list(layer) if K is Mla else (list(layer[2:]) if layer[0] == "kv" else [])      # the position-indexed row arrays of a layer
    n_checked = 0
    for layer, ref_layer in zip(got, want[95]):
        for a, b in zip(parts(layer), parts(ref_layer)):
            assert np.array_equal(a[:64], b[:64]) and not a[64:].any() and b[64:].any()
            n_checked += 1
    assert n_checked >= 2


# ---- 8: production width -------------------------------------------------------------------------------------------------------------------------------
def test_production_width_pages_of_64():
    """QCN widths (hidden 2048, top-10 of 72, head_dim 256, 16 query heads on 2 KV heads), page_tokens 64, rows crossing positions 64 and 128"""
    st, eng, orc, keep, d = build(seed=23, dims=(2048, 512, 72, 10, 512, 512), hd=256, nh=16, kv_max=160, kinds=["la", "gqa"])
    rng = np.random.default_rng(2)
    prompts = [_toks(rng, d, n) for n in (126, 3, 62)]
    firsts = _toks(rng, d, 3)
    refs = [seq._reference(st, d, p, f, 4) for p, f in zip(prompts, firsts)]
    st.create_slots(3, 150, page_tokens=64, n_pages=6)
    for s, p in enumerate(prompts):
        st.prefill_slot(s, p, chunk=50)
    toks, pos = list(firsts), [len(p) for p in prompts]
    for k in range(4):
        ids, lg = st.step_multi([0, 1, 2], toks, pos, logits=True)
        for i, (ref, _) in enumerate(refs):
            assert np.array_equal(lg[i].view(U), ref[k][0]), ("logits", k, i)
            assert ids[i] == ref[k][1]
        toks = ids; pos = [p + 1 for p in pos]
    assert st.slot_pages() == dict(page_tokens=64, n_pages=6, free=0, per_slot=[3, 1, 2])
    for i, (_, snap) in enumerate(refs):
        _same(_slot_state(Gqa, st, d, i, pos[i]), snap)


# ---- 9: refusals ---------------------------------------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing():
    st, keep, d = Gqa.build(kv_max=128)
    st.create_slots(3, 100)
    st.fill_state_synthetic(d["kv_max"], seed=5)
    st.save_slot(1, 40)
    want = _snap(st, d, 40)
    assert st.slot_pages() == dict(page_tokens=0, n_pages=0, free=0, per_slot=[0, 0, 0])      # flat slots
    for bad in (dict(page_tokens=0, n_pages=4), dict(page_tokens=24, n_pages=4), dict(page_tokens=16, n_pages=4), dict(page_tokens=48, n_pages=4),
                dict(page_tokens=32, n_pages=0)):
        with pytest.raises(ValueError) as e:
            st.create_slots(3, 100, **bad)
        assert ("n_pages" if bad["n_pages"] == 0 else "page_tokens") in str(e.value)
        _same(_slot_state(Gqa, st, d, 1, 40), want)            # the earlier slots are still there
    st.trim_slot(1, 0)                                          # flat slots: a no-op that still checks its arguments
    _same(_slot_state(Gqa, st, d, 1, 40), want)
    for slot, n in ((3, 0), (-1, 0), (1, -1), (1, 101)):
        with pytest.raises(ValueError):
            st.trim_slot(slot, n)

    st.create_slots(3, 100, page_tokens=PT, n_pages=6)
    st.fill_state_synthetic(d["kv_max"], seed=5)
    st.save_slot(1, 40)
    before = st.slot_pages()
    assert before["per_slot"] == [0, 2, 0]

    def unchanged():
        assert st.slot_pages() == before
        _same(_slot_state(Gqa, st, d, 1, 40), want)

    for slot, n in ((3, 0), (-1, 0), (1, -1), (1, 101)):
        with pytest.raises(ValueError):
            st.trim_slot(slot, n)
    unchanged()
    st.set_option("multi_attn_fast", 1)                         # the split-KV form does not read pages: refused by name, not silently ignored
    calls = [lambda: st.step_multi([1], [2], [40]), lambda: st.extend_multi([0], [[1, 2]], [0]), lambda: st.generate_multi([1], [2], [40], 4),
             lambda: st.verify_multi([1], [[2, 3]], [40]), lambda: st.generate_multi_lookup([1], [2], [40], 4)]
    for call in calls:
        _state_error(call, "multi_attn_fast", "paged")
    unchanged()
    st.set_option("multi_attn_fast", 0)
    st.verify_multi([1], [[2, 3, 4]], [40])                     # pending: trim is refused with the other slot calls
    pending = st.slot_pages()
    _state_error(lambda: st.trim_slot(1, 0), "pending")
    assert st.slot_pages() == pending
    st.commit_multi([0])
    _same(_slot_state(Gqa, st, d, 1, 40), want)
    st.set_kv_dtype(True)                                       # the pools hold FP16 rows, the store now E4M3
    st.reset_decode_state(d["kv_max"])
    for call in (lambda: st.step_multi([1], [2], [40]), lambda: st.load_slot(1, 40), lambda: st.trim_slot(1, 0), lambda: st.slot_pages()):
        _state_error(call, "E4M3")
    st.set_kv_dtype(False)
    unchanged()
