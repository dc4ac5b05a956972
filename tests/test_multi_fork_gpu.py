"""Slot fork with shared, copy-on-write pages (kr_decode_slot_fork / kr_decode_slot_page_ids; docs/design/22-slot-fork.md): after fork_slot(src, dsts,
seq_len) every dst behaves as a fresh slot into which src's first seq_len positions were prefilled.  The reference is never the forked path itself: it is
the single-sequence path (decode_step, generate_batch, prefill + state read-back, through the Gqa / Mla helpers of tests/test_multi_paged_gpu.py), or the
same call sequence on flat slots, which copy everything and share nothing.  Every assertion is on ids and on u32 / stored-row bit patterns."""
import numpy as np
import pytest

from tests import test_multi_mla_gpu as mla
from tests import test_multi_seq_gpu as seq
from tests.test_decode_gpu import build
from tests.test_multi_paged_gpu import PT, Gqa, Mla, _pages, _slot_state, _state_error, _toks
from tests.test_speculative_gpu import _same

pytestmark = pytest.mark.gpu
U = np.uint32
SRC, DSTS = 2, [0, 3]
ALL = [SRC] + DSTS


def _ids(st, slot):
    return st.slot_page_ids(slot)


def _tables(st, n_slots=4):
    return [_ids(st, s) for s in range(n_slots)], st.slot_pages()


def _steps(st, slots, toks, pos, refs, n_steps, k0=0):
    """n_steps of step_multi over the slots: row i's logits and id are step k0 + k of refs[i]; returns the next tokens and positions"""
    toks, pos = list(toks), list(pos)
    for k in range(n_steps):
        ids, lg = st.step_multi(slots, toks, pos, logits=True)
        for i, (ref, _) in enumerate(refs):
            assert np.array_equal(lg[i].view(U), ref[k0 + k][0]), ("logits", k, i)
            assert ids[i] == ref[k0 + k][1], ("id", k, i)
        toks = ids; pos = [p + 1 for p in pos]
    return toks, pos


def _rows(K, layer):
    """the position-indexed row arrays of one layer of a snapshot (MLA: latent and rope-key rows; hybrid: K and V rows of a GQA layer)"""
    return list(layer) if K is Mla else (list(layer[2:]) if layer[0] == "kv" else [])


# ---- 1, 2: a fork in the middle of a page and one at a page edge, then 40 steps with three different first tokens crossing position 96 -------------------
def _fork_then_steps(K, st, d, n_prompt, n_pages=10, n_steps=40):
    rng = np.random.default_rng(71)
    prompt, firsts = _toks(rng, d, n_prompt), _toks(rng, d, 3)
    refs = [K.reference(st, d, prompt, f, n_steps) for f in firsts]
    st.create_slots(4, 120, page_tokens=PT, n_pages=n_pages)
    st.prefill_slot(SRC, prompt, chunk=24)
    free = st.slot_pages()["free"]
    assert free == n_pages - _pages(n_prompt)
    src_ids = _ids(st, SRC)
    st.fork_slot(SRC, DSTS, n_prompt)
    full, part = n_prompt // PT, n_prompt % PT
    got = [_ids(st, s) for s in ALL]
    assert got[0][0] == src_ids[0], "src's table row is what it was"
    for ids, refc in got:
        assert ids[:full] == src_ids[0][:full] and refc[:full] == [3] * full      # whole pages below the fork point: shared, three holders
        assert all(i == -1 for i in ids[full + (1 if part else 0):])               # later pages are unmapped
    if part:      # the boundary page: one of its own per slot, one reference each
        edge = [ids[full] for ids, _ in got]
        assert len(set(edge)) == 3 and min(edge) >= 0 and [refc[full] for _, refc in got] == [1, 1, 1]
    assert st.slot_pages()["free"] == free - (2 if part else 0)
    assert st.slot_pages()["per_slot"] == [_pages(n_prompt), 0, _pages(n_prompt), _pages(n_prompt)]
    toks, pos = _steps(st, ALL, firsts, [n_prompt] * 3, refs, 1)
    if not part:      # the first step maps one page per slot
        assert st.slot_pages()["free"] == free - 3 and [_ids(st, s)[1][full] for s in ALL] == [1, 1, 1]
    toks, pos = _steps(st, ALL, toks, pos, refs, n_steps - 1, 1)
    for ids, refc in (_ids(st, s) for s in ALL):      # appending never touched the shared pages
        assert ids[:full] == src_ids[0][:full] and refc[:full] == [3] * full
    assert st.slot_pages()["free"] == n_pages - full - 3 * (_pages(pos[0]) - full)
    for i, (_, snap) in enumerate(refs):
        K.same(_slot_state(K, st, d, ALL[i], pos[i]), snap)


@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("n_prompt", [70, 64])
def test_hybrid_fork_and_steps_equal_decode_step_alone(n_prompt, fp8):
    st, keep, d = Gqa.build(fp8, seed=3, hd=64, nh=4, kv_max=128)
    _fork_then_steps(Gqa, st, d, n_prompt)


@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("cfg,n_prompt", [(mla.CFGS[0], 70), (mla.CFGS[1], 70), (mla.CFGS[2], 70), (mla.CFGS[0], 64)])
def test_mla_fork_and_steps_equal_decode_step_alone(cfg, n_prompt, fp8):
    st, keep, d = Mla.build(fp8, kv_max=128, **cfg)
    _fork_then_steps(Mla, st, d, n_prompt)


# ---- 3: short forks: nothing is shared -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [Gqa, Mla])
def test_short_forks_share_nothing(K):
    st, keep, d = K.build(kv_max=128)
    rng = np.random.default_rng(72)
    prompt, other, firsts = _toks(rng, d, 31), _toks(rng, d, 40), _toks(rng, d, 3)
    fresh = K.reference(st, d, [], firsts[0], 4)
    refs = [K.reference(st, d, prompt, f, 5) for f in firsts]
    st.create_slots(4, 120, page_tokens=PT, n_pages=8)
    st.prefill_slot(0, other, chunk=24)                          # the dst holds another sequence; slot 1 was never used
    st.fork_slot(1, 0, 0)                                         # an int for dsts
    assert st.slot_pages()["free"] == 8 and _ids(st, 0) == ([-1] * 4, [0] * 4)
    toks, pos = _steps(st, [0], firsts[:1], [0], [fresh], 4)      # the dst equals a fresh slot
    K.same(_slot_state(K, st, d, 0, 4), fresh[1])
    st.trim_slot(0, 0)
    st.prefill_slot(SRC, prompt, chunk=24)
    st.fork_slot(SRC, DSTS, 31)
    edge = [_ids(st, s) for s in ALL]
    assert len({ids[0] for ids, _ in edge}) == 3 and all(refc == [1, 0, 0, 0] and ids[1:] == [-1] * 3 for ids, refc in edge)
    assert st.slot_pages()["free"] == 5
    toks, pos = _steps(st, ALL, firsts, [31] * 3, refs, 5)        # over position 32
    for i, (_, snap) in enumerate(refs):
        K.same(_slot_state(K, st, d, ALL[i], pos[i]), snap)


# ---- 4: rows at or past the fork point read as zero ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,fp8", [(Gqa, False), (Gqa, True), (Mla, False), (Mla, True)])
def test_rows_past_the_fork_point_are_zero(K, fp8):
    st, keep, d = K.build(fp8, kv_max=128)
    rng = np.random.default_rng(73)
    prompt = _toks(rng, d, 90)
    K.start(st, d, prompt)
    want = K.snap(st, d, 96)                                      # the single-sequence rows of the 90 positions
    out = []
    for paged in (True, False):
        st.create_slots(4, 120, **(dict(page_tokens=PT, n_pages=8) if paged else {}))
        st.prefill_slot(SRC, prompt[:70], chunk=24)
        st.prefill_slot(SRC, prompt[70:], 70, chunk=24)           # src runs on to position 90
        st.prefill_slot(0, prompt[:80], chunk=24)                 # the dst is dirty past the fork point
        st.fork_slot(SRC, 0, 70)
        if paged:
            assert _ids(st, 0)[1] == [2, 2, 1, 0] and _ids(st, SRC)[1] == [2, 2, 1, 0] and st.slot_pages()["free"] == 8 - 4
        K.start(st, d, prompt)                                    # the store's rows are non-zero before the load
        st.load_slot(0, 96)
        out.append(K.snap(st, d, 96))
        src = _slot_state(K, st, d, SRC, 90)
        n_checked = 0
        for got, ref, own in zip(out[-1], want, src):
            for a, b, c in zip(_rows(K, got), _rows(K, ref), _rows(K, own)):
                assert np.array_equal(a[:70], b[:70]) and np.array_equal(a[:70], c[:70]) and not a[70:].any() and b[70:90].any()
                assert np.array_equal(c[:90], b[:90])              # src is unchanged
                n_checked += 1
        assert n_checked >= 2
    for got, flat in zip(*out):
        for a, b in zip(_rows(K, got), _rows(K, flat)):
            assert np.array_equal(a, b)


# ---- 5: a write below the fork point lands in a private copy --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg,fp8", [(mla.CFGS[0], False), (mla.CFGS[2], True)])
def test_write_below_the_fork_point_copies_the_page(cfg, fp8):
    st, keep, d = Mla.build(fp8, kv_max=128, **cfg)
    rng = np.random.default_rng(74)
    prompt, new, firsts = _toks(rng, d, 70), _toks(rng, d, 20), _toks(rng, d, 2)
    src_ref = Mla.reference(st, d, prompt, firsts[0], 6)
    dst_ref = Mla.reference(st, d, prompt[:40] + new, firsts[1], 6)
    st.create_slots(4, 120, page_tokens=PT, n_pages=8)
    st.prefill_slot(SRC, prompt, chunk=24)
    st.fork_slot(SRC, 0, 70)
    before, free = _ids(st, 0), st.slot_pages()["free"]
    assert before[1] == [2, 2, 1, 0] and free == 4
    st.extend_multi([0], [new], [40])                             # positions [40, 60): all in page 1
    after, src = _ids(st, 0), _ids(st, SRC)
    assert after[0][0] == before[0][0] and after[0][2] == before[0][2] and after[0][1] not in (before[0][1], -1)
    assert after[1] == [2, 1, 1, 0] and src[0][:2] == before[0][:2] and src[1] == [2, 1, 1, 0]      # the old page 1 has one reference fewer
    assert st.slot_pages()["free"] == free - 1
    _steps(st, [SRC, 0], firsts, [70, 60], [src_ref, dst_ref], 6)
    Mla.same(_slot_state(Mla, st, d, SRC, 76), src_ref[1])
    Mla.same(_slot_state(Mla, st, d, 0, 66), dst_ref[1])


# ---- 6: speculation on forked slots ----------------------------------------------------------------------------------------------------------------------
SAMPLER = dict(temperature=[0.0, 0.8, 1.0], top_k=[0, 20, 0], top_p=[1.0, 0.9, 1.0], presence_penalty=[1.5, 0.0, 0.5], rng_seeds=[7, 8, 9])


def _speculation(K, st, d, paged, prompt, firsts):
    out = []
    for sampler in (None, SAMPLER):
        st.create_slots(4, 120, **(dict(page_tokens=PT, n_pages=12) if paged else {}))
        st.prefill_slot(SRC, prompt, chunk=24)
        st.fork_slot(SRC, DSTS, len(prompt))
        ctx, pos = [prompt + prompt] * 3, [len(prompt)] * 3
        if sampler:
            T = st.generate_multi_lookup_sample(ALL, firsts, pos, 14, ctx, 7, 2, **sampler)
        else:
            T = st.generate_multi_lookup(ALL, firsts, pos, 14, ctx, 7, 2)
        if paged:      # what the call mapped past each row's end went back; the whole page below the fork point is still shared
            assert [st.slot_pages()["per_slot"][s] for s in ALL] == [_pages(len(prompt) + len(t)) for t in T]
            assert all(_ids(st, s)[1][0] == 3 for s in ALL)
        out.append((T, dict(st.last_multi_lookup_stats), [_slot_state(K, st, d, s, len(prompt) + len(t)) for s, t in zip(ALL, T)],
                    [st.slot_sampler_state(s) for s in ALL]))
    return out


@pytest.mark.parametrize("K", [Gqa, Mla])
def test_speculation_on_forked_slots_equals_the_flat_run(K):
    st, keep, d = K.build(kv_max=128)
    rng = np.random.default_rng(75)
    prompt, firsts = _toks(rng, d, 60), _toks(rng, d, 3)          # runs of 8 from 60 straddle position 64
    truth = []
    for f in firsts:
        K.start(st, d, prompt); truth.append(st.generate_batch(f, len(prompt), 14))
    got = _speculation(K, st, d, True, prompt, firsts)
    flat = _speculation(K, st, d, False, prompt, firsts)
    assert len(got) == len(flat) == 2
    for (a, b, states, smp), (fa, fb, fstates, fsmp) in zip(got, flat):
        assert a == fa and b == fb
        for x, y in zip(states, fstates):
            K.same(x, y)
        for (seen, r), (fseen, fr) in zip(smp, fsmp):
            assert np.array_equal(seen, fseen) and r == fr
    assert got[0][0] == truth                                     # generate_multi_lookup = generate_batch on each sequence alone


# ---- 7: a page goes back with its last reference ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,fp8", [(Gqa, False), (Mla, True)])
def test_last_reference_frees(K, fp8):
    st, keep, d = K.build(fp8, kv_max=128)
    rng = np.random.default_rng(76)
    prompt, firsts, probe = _toks(rng, d, 70), _toks(rng, d, 2), _toks(rng, d, 1)[0]
    refs = [K.reference(st, d, prompt, f, 3) for f in firsts]
    st.create_slots(4, 120)
    flat = st.step_multi([1], [probe], [40], logits=True)         # what a fresh flat slot gives
    st.create_slots(4, 120, page_tokens=PT, n_pages=6)
    st.prefill_slot(SRC, prompt, chunk=24)
    st.fork_slot(SRC, DSTS, 70)
    assert st.slot_pages()["free"] == 1
    st.trim_slot(SRC, 0)                                          # src's own boundary page comes back; the shared pages stay, two holders each
    assert st.slot_pages()["free"] == 2 and st.slot_pages()["per_slot"] == [3, 0, 0, 3]
    assert _ids(st, 0)[1] == [2, 2, 1, 0] and _ids(st, 0)[0][:2] == _ids(st, 3)[0][:2]
    toks, pos = _steps(st, DSTS, firsts, [70, 70], refs, 3)
    for i, (_, snap) in enumerate(refs):
        K.same(_slot_state(K, st, d, DSTS[i], 73), snap)
    st.trim_slot(0, 0)
    assert st.slot_pages()["free"] == 3 and _ids(st, 3)[1] == [1, 1, 1, 0]
    st.trim_slot(3, 0)
    assert st.slot_pages()["free"] == 6 and st.slot_pages()["per_slot"] == [0, 0, 0, 0]
    ids, lg = st.step_multi([1], [probe], [40], logits=True)      # a never-filled slot maps two of the dirty pages: they must read as zero
    assert st.slot_pages()["per_slot"] == [0, 2, 0, 0]
    assert np.array_equal(lg.view(U), flat[1].view(U)) and ids == flat[0]


# ---- 8: the pages a dst held are released and counted ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [Gqa, Mla])
def test_pages_of_the_dsts_count_towards_the_fork(K):
    st, keep, d = K.build(kv_max=128)
    rng = np.random.default_rng(77)
    prompt, other, firsts = _toks(rng, d, 70), _toks(rng, d, 33), _toks(rng, d, 5)
    refs = [K.reference(st, d, prompt, f, 2) for f in firsts[:4]]
    other_ref = K.reference(st, d, other, firsts[4], 1)
    dsts = [0, 3, 1]                                              # three boundary pages; slot 0 holds two pages of another sequence

    def fill(n_pages):
        st.create_slots(4, 120, page_tokens=PT, n_pages=n_pages)
        st.prefill_slot(SRC, prompt, chunk=24)
        st.prefill_slot(0, other, chunk=24)

    fill(5)                                                       # nothing free, two to come: one page short
    before = _tables(st)
    assert before[1]["free"] == 0
    _state_error(lambda: st.fork_slot(SRC, dsts, 70), "3 more pages", "2 of 5")
    assert _tables(st) == before                                  # nothing was released, nothing mapped
    _steps(st, [SRC, 0], [firsts[0], firsts[4]], [70, 33], [refs[0], other_ref], 1)
    fill(6)                                                       # one free and two to come: it fits only because of them
    assert st.slot_pages()["free"] == 1
    st.fork_slot(SRC, dsts, 70)
    pages = st.slot_pages()
    assert pages["free"] == 0 and pages["per_slot"] == [3, 3, 3, 3]
    assert all(_ids(st, s)[1] == [4, 4, 1, 0] for s in range(4))
    slots = [SRC] + dsts
    _steps(st, slots, firsts[:4], [70] * 4, refs, 2)
    for i, (_, snap) in enumerate(refs):
        K.same(_slot_state(K, st, d, slots[i], 72), snap)


# ---- 9: a private copy that the pool cannot give refuses the whole call ---------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [Gqa, Mla])
def test_copy_on_write_without_a_free_page_is_refused_whole(K):
    st, keep, d = K.build(kv_max=128)
    rng = np.random.default_rng(78)
    prompt, first = _toks(rng, d, 70), _toks(rng, d, 1)[0]
    ref = K.reference(st, d, prompt, first, 2)
    st.create_slots(4, 120, page_tokens=PT, n_pages=4)
    st.prefill_slot(SRC, prompt, chunk=24)
    st.fork_slot(SRC, 0, 70)
    before = _tables(st)
    assert before[1]["free"] == 0
    # row 1 writes position 40 of slot 0, inside shared page 1: it needs a private copy and there is no page
    _state_error(lambda: st.step_multi([SRC, 0], [first, first], [70, 40]), "row 1", "slot 0", "0 of 4")
    _state_error(lambda: st.verify_multi([0], [[first, first]], [62]), "row 0")
    _state_error(lambda: st.generate_multi([SRC, 0], [first, first], [70, 50], 4), "row 1")
    assert _tables(st) == before
    _steps(st, [SRC, 0], [first, first], [70, 70], [ref, ref], 2)      # row 0 of the refused call had not advanced: both slots still step as the reference
    K.same(_slot_state(K, st, d, SRC, 72), ref[1])
    K.same(_slot_state(K, st, d, 0, 72), ref[1])


# ---- 10: n-best sampling is a fork and four seeds --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [Gqa, Mla])
def test_n_best_equals_generate_batch_per_seed(K):
    st, keep, d = K.build(kv_max=128)
    rng = np.random.default_rng(79)
    prompt, first = _toks(rng, d, 45), _toks(rng, d, 1)[0]
    T, TK, TP, PEN, seeds, L = 0.8, 20, 0.9, 0.5, [11, 12, 13, 14], 10
    truth = []
    for seed in seeds:
        K.start(st, d, prompt); truth.append(st.generate_batch(first, len(prompt), L, T, TK, TP, (), PEN, rng_seed=seed))
    assert len({tuple(t) for t in truth}) > 1                     # the seeds draw different continuations
    st.create_slots(5, 120, page_tokens=PT, n_pages=12)
    st.prefill_slot(4, prompt, chunk=24)
    dsts = [0, 1, 2, 3]
    st.fork_slot(4, dsts, 45)
    for s, seed in zip(dsts, seeds):
        st.set_slot_sampler(s, first, T, TK, TP, PEN, seed)
    toks, got = [first] * 4, [[] for _ in dsts]
    for k in range(L):
        toks = st.step_multi_sample(dsts, toks, [45 + k] * 4)
        for g, t in zip(got, toks):
            g.append(t)
    assert got == truth
    states = [st.slot_sampler_state(s) for s in dsts]
    st.fork_slot(4, dsts, 45)                                     # again, onto slots that hold the earlier run: src is what it was, the samplers are not touched
    for s, (seen, r) in zip(dsts, states):
        seen2, r2 = st.slot_sampler_state(s)
        assert np.array_equal(seen, seen2) and r == r2
    assert st.slot_pages()["per_slot"] == [2, 2, 2, 2, 2] and _ids(st, 4)[1][:2] == [5, 1]
    assert st.generate_multi(dsts, [first] * 4, [45] * 4, L, (), T, TK, TP, PEN, seeds) == truth


# ---- 11: every refusal changes nothing -------------------------------------------------------------------------------------------------------------------
def test_refusals_change_nothing():
    st, keep, d = Gqa.build(kv_max=128)
    rng = np.random.default_rng(80)
    prompt, other = _toks(rng, d, 40), _toks(rng, d, 20)
    Gqa.start(st, d, prompt); want = Gqa.snap(st, d, 40)
    Gqa.start(st, d, other); want0 = Gqa.snap(st, d, 20)
    bad = [(4, [0]), (-1, [0]), (2, [4]), (2, [-1]), (2, [2]), (2, [0, 2]), (2, [0, 0]), (2, []), (2, [0, 1, 3, 0])]
    for paged in (True, False):
        st.create_slots(4, 100, **(dict(page_tokens=PT, n_pages=6) if paged else {}))
        st.prefill_slot(SRC, prompt, chunk=24)
        st.prefill_slot(0, other, chunk=24)
        before = _tables(st) if paged else None

        def unchanged():
            if paged:
                assert _tables(st) == before
            _same(_slot_state(Gqa, st, d, SRC, 40), want)
            _same(_slot_state(Gqa, st, d, 0, 20), want0)

        for src, dsts in bad:
            with pytest.raises(ValueError):
                st.fork_slot(src, dsts, 40)
        for n in (-1, 101):
            with pytest.raises(ValueError) as e:
                st.fork_slot(SRC, [0], n)
            assert "seq_len" in str(e.value)
        for name, call in (("src", lambda: st.fork_slot(4, [0], 40)), ("dsts[1]", lambda: st.fork_slot(2, [0, 2], 40)),
                           ("dsts[1]", lambda: st.fork_slot(2, [0, 0], 40)), ("n_dst", lambda: st.fork_slot(2, [], 40))):
            with pytest.raises(ValueError) as e:
                call()
            assert name in str(e.value)
        with pytest.raises(ValueError):
            st.slot_page_ids(4)
        unchanged()
        st.verify_multi([SRC], [[2, 3, 4]], [40])                 # pending: fork is refused with the other slot calls
        pending = _tables(st) if paged else None
        _state_error(lambda: st.fork_slot(SRC, [0], 40), "pending")
        if paged:
            assert _tables(st) == pending
        st.commit_multi([0])
        unchanged()
        if not paged:
            _state_error(lambda: st.slot_page_ids(0), "flat")


# ---- 11b: a fork whose source page still waits for its own copy ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fp8", [False, True])
def test_fork_out_of_a_page_whose_copy_is_still_queued(fp8):
    """slot 0, forked from slot 2, gets a private copy of page 1 queued by a call that reserves and opens no pass (generate_multi of 0 tokens); forking slot 0
    inside that page must copy it only after it was written -- both destination pages held another sequence's rows before"""
    st, keep, d = Mla.build(fp8, kv_max=128)
    rng = np.random.default_rng(82)
    prompt, other, first = _toks(rng, d, 70), _toks(rng, d, 64), _toks(rng, d, 1)[0]
    ref = Mla.reference(st, d, prompt[:40], first, 4)
    Mla.start(st, d, prompt)
    whole = Mla.snap(st, d, 70)
    want = [(ck[:40], kp[:40]) for ck, kp in whole]
    st.create_slots(4, 120, page_tokens=PT, n_pages=8)
    st.prefill_slot(1, other, chunk=24)                          # pages 0 and 1
    st.prefill_slot(SRC, prompt, chunk=24)                       # pages 2, 3, 4
    st.fork_slot(SRC, 0, 70)                                     # slot 0: [2, 3, 5]
    st.trim_slot(1, 0)                                           # pages 0 and 1 are free and dirty
    assert st.generate_multi([0], [first], [40], 0) == [[]]      # reserves position 40: page 0 becomes slot 0's copy of page 3, and no pass opens
    assert _ids(st, 0) == ([2, 0, 5, -1], [2, 1, 1, 0]) and _ids(st, SRC)[1] == [2, 1, 1, 0]
    st.fork_slot(0, 3, 40)                                       # page 1 <- rows [32, 40) of page 0, queued behind page 0 <- page 3
    assert _ids(st, 3) == ([2, 1, -1, -1], [3, 1, 0, 0]) and st.slot_pages()["free"] == 2
    Mla.start(st, d, other)                                      # the store's rows are another sequence's before the load
    st.load_slot(3, 64)
    got = Mla.snap(st, d, 64)
    for layer, ref_layer in zip(got, want):
        for a, b in zip(layer, ref_layer):
            assert np.array_equal(a[:40], b) and not a[40:].any()
    _steps(st, [3], [first], [40], [ref], 4)
    Mla.same(_slot_state(Mla, st, d, 3, 44), ref[1])
    Mla.same(_slot_state(Mla, st, d, 0, 70), whole)             # slot 0 holds the whole prompt, page 0 with the rows of page 3
    Mla.same(_slot_state(Mla, st, d, SRC, 70), whole)


# ---- 11c: the copy kernel at every split, on one pool ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("row_bytes,page_tokens,offset", [(5, 32, 0), (24, 32, 0), (64, 32, 0), (256, 32, 0), (1, 16, 0), (20, 1, 0), (5, 32, 4), (3, 7, 0), (4100, 1, 0)])
def test_copy_kernel_at_every_split(row_bytes, page_tokens, offset):
    """kr_multi_copy_pages_kernel through its test aid against numpy: rows copied, zeroes behind them, the other pages untouched -- row sizes whose split falls
    inside a 16-byte vector (5, 24, 1), on one (64, 256), pages that are not 16-byte aligned (20, 21, 4100 bytes; a pool 4 bytes off), more than one sweep
    of the block (8192 and 4100 bytes)"""
    from krasis_amd._lib import check, load_library
    lib = load_library()
    page_bytes = row_bytes * page_tokens
    splits = list(range(page_tokens + 1))                        # every number of rows, none and all among them
    n = len(splits)
    rng = np.random.default_rng(83)
    pool = rng.integers(1, 256, (2 * n + 1, page_bytes), dtype=np.uint8)      # no zero byte: a zero in the result was written
    want = pool.copy()
    dst = np.arange(n, dtype=np.int32)[::-1].copy() * 2 + 1      # odd pages, in falling order
    src = np.arange(n, dtype=np.int32) * 2
    rows = np.array(splits, np.int32)
    for dpg, spg, r in zip(dst, src, rows):
        want[dpg, :r * row_bytes] = pool[spg, :r * row_bytes]; want[dpg, r * row_bytes:] = 0
    got = pool.copy()
    check(lib.kr_copy_pages(got.ctypes.data, page_bytes, len(pool), page_tokens, n, dst.ctypes.data, src.ctypes.data, rows.ctypes.data, offset))
    assert np.array_equal(got, want)
    for bad in ((dst, dst, rows), (dst, src, rows + page_tokens + 1), (np.ones(n, np.int32), src, rows), (dst + 2 * n, src, rows)):
        with pytest.raises(ValueError):
            check(lib.kr_copy_pages(got.ctypes.data, page_bytes, len(pool), page_tokens, n, *(np.ascontiguousarray(x, np.int32).ctypes.data for x in bad), offset))
    assert np.array_equal(got, want)


# ---- 12: production width --------------------------------------------------------------------------------------------------------------------------------
def test_production_width_fork_in_pages_of_64():
    """QCN widths (hidden 2048, top-10 of 72, head_dim 256, 16 query heads on 2 KV heads), page_tokens 64: a fork at 126, inside the second page, then
    steps over position 128"""
    st, eng, orc, keep, d = build(seed=23, dims=(2048, 512, 72, 10, 512, 512), hd=256, nh=16, kv_max=160, kinds=["la", "gqa"])
    rng = np.random.default_rng(81)
    prompt, firsts = _toks(rng, d, 126), _toks(rng, d, 3)
    refs = [seq._reference(st, d, prompt, f, 4) for f in firsts]
    st.create_slots(3, 150, page_tokens=64, n_pages=7)
    st.prefill_slot(1, prompt, chunk=50)
    st.fork_slot(1, [0, 2], 126)
    assert [st.slot_page_ids(s)[1] for s in range(3)] == [[3, 1, 0]] * 3 and st.slot_pages()["free"] == 3
    toks, pos = _steps(st, [1, 0, 2], firsts, [126] * 3, refs, 4)
    assert st.slot_pages() == dict(page_tokens=64, n_pages=7, free=0, per_slot=[3, 3, 3])
    for i, (_, snap) in enumerate(refs):
        _same(_slot_state(Gqa, st, d, [1, 0, 2][i], 130), snap)
