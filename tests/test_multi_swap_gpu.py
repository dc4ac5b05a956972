"""Slot export and import (kr_decode_slots_export / kr_decode_slots_import, docs/design/38-slot-swap.md): a slot's complete state goes out to host memory as one
self-describing image and comes back into any slot of any compatible slot set, bit for bit -- flat or paged, any page size and placement, pages shared by fork.
Every assertion is on ids, byte arrays and u32 bit patterns, and the reference is never the new path: it is the single-sequence path (K.reference), the state
read back through load_slot + get_decode_state (_slot_state), or the same calls without a swap in between."""
import functools

import numpy as np
import pytest

from krasis_amd.decode_store import slot_image_info
from tests import test_multi_mla_gpu as mla
from tests.test_multi_paged_gpu import PT, Gqa, Mla, _pages, _slot_state, _state_error, _toks

pytestmark = pytest.mark.gpu
U = np.uint32
MAXSEQ = 120
MODELS = [(k, fp8) for k in ("gqa", "mla", "mla256") for fp8 in (False, True)]
BUILD = {"gqa": (Gqa, dict(seed=3, hd=64, nh=4)), "mla": (Mla, mla.CFGS[0]), "mla256": (Mla, mla.CFGS[2])}
assert mla.CFGS[2]["klr"] == 256
FLAT, P32, P64 = {}, dict(page_tokens=PT, n_pages=10), dict(page_tokens=64, n_pages=6)


@functools.lru_cache(maxsize=None)
def _model(kind, fp8):
    """one store per model and KV element type, shared by the tests (each creates its own slots), with the single-sequence references computed once"""
    K, cfg = BUILD[kind]
    st, keep, d = K.build(fp8, kv_max=128, **cfg)
    rng = np.random.default_rng(11)
    P = dict(a=_toks(rng, d, 70), b=_toks(rng, d, 40), c=_toks(rng, d, 40))
    P["a40"] = P["a"][:40]
    F = dict(zip(("a", "a40", "b", "c"), _toks(rng, d, 4)))
    R = dict(a=K.reference(st, d, P["a"], F["a"], 45), a40=K.reference(st, d, P["a40"], F["a40"], 30), b=K.reference(st, d, P["b"], F["b"], 20),
             c=K.reference(st, d, P["c"], F["c"], 20))
    K.start(st, d, P["a"]); R["a70"] = K.snap(st, d, 70)
    K.start(st, d, P["b"]); R["b40"] = K.snap(st, d, 40)
    return K, st, keep, d, P, F, R


def _steps(st, slots, toks, pos, n, refs=None, off=None):
    """n greedy steps of the slots together; against refs[i][0][off[i] + k] (logits bits, id) where given"""
    toks, pos = list(toks), list(pos)
    for k in range(n):
        ids, lg = st.step_multi(slots, toks, pos, logits=True)
        for i in range(len(slots)):
            if refs is not None:
                want = refs[i][0][off[i] + k]
                assert np.array_equal(lg[i].view(U), want[0]), ("logits", k, i)
                assert ids[i] == want[1], ("id", k, i)
        toks = ids; pos = [p + 1 for p in pos]
    return toks, pos


def _sections(img):
    """the sections of an image, found through its header and table alone"""
    assert img.dtype == np.uint8 and img.size % 16 == 0
    h = img[:64].view(U)
    assert h[0] == 0x49534C53 and h[1] == 1 and int(img[40:48].view(np.uint64)[0]) == img.size and h[13] == 64
    tab = img[64:64 + 16 * int(h[12])].view(np.uint64).reshape(-1, 2)
    assert all(int(o) % 16 == 0 for o, _ in tab)
    return [img[int(o):int(o) + int(b)] for o, b in tab]


def _pairs(K, snap):
    return [(e[2], e[3]) if K is Gqa else e for e in snap]


def _image_equals_state(K, img, snap, sampler=0):
    """every section, byte for byte, against what load_slot + get_decode_state gave for that layer, cut to seq_len"""
    secs, pairs = _sections(img), _pairs(K, snap)
    assert len(secs) == 2 * len(pairs) + sampler
    for li, (x, y) in enumerate(pairs):
        assert secs[2 * li].tobytes() == np.ascontiguousarray(x).tobytes(), ("layer", li, "a")
        assert secs[2 * li + 1].tobytes() == np.ascontiguousarray(y).tobytes(), ("layer", li, "b")


def _tables(st, n):
    return [st.slot_page_ids(s) for s in range(n)], st.slot_pages()


def _chunk(st, v):
    st.set_option("slot_swap_chunk_bytes", v if v else 4 << 20)      # 0: the default


# ---- 1: the image against the old route ------------------------------------------------------------------------------------------------------------------
def _export_three_ways(K, st, d, P, F, name, n):
    """prefill_slot of n tokens, 5 steps, export: on flat slots, pages of 32 and pages of 64 -> the three images (each checked against load_slot + get_state)"""
    out = []
    for geo, slot in ((FLAT, 1), (P32, 2), (P64, 0)):
        st.create_slots(4, MAXSEQ, **geo)
        st.prefill_slot(slot, P[name][:n], chunk=24)
        _steps(st, [slot], [F[name]], [n], 5)
        before = _tables(st, 4) if geo else None
        assert st.slot_image_bytes(n + 5) == st.export_slot(slot, n + 5).size
        img = st.export_slot(slot, n + 5)
        info = slot_image_info(img)
        assert (info["seq_len"], info["kv_fp8"], info["has_sampler"]) == (n + 5, bool(d.get("fp8")), False)
        _image_equals_state(K, img, _slot_state(K, st, d, slot, n + 5))
        if geo:
            assert _tables(st, 4) == before
        out.append(img)
    return out


@pytest.mark.parametrize("kind,fp8", MODELS)
def test_image_equals_load_slot_and_get_state(kind, fp8):
    K, st, keep, d, P, F, R = _model(kind, fp8)
    for n in (70, 64):      # mid-page, and a page edge
        flat, p32, p64 = _export_three_ways(K, st, d, P, F, "a", n)
        assert flat.tobytes() == p32.tobytes() == p64.tobytes(), n      # canonical: nothing of the slot set in it


# ---- 2: round trip under another placement -----------------------------------------------------------------------------------------------------------------
def _round_trip(K, st, d, P, F, R, src, dst):
    """sequence a: 70 tokens + 5 steps in a slot of `src`, exported with release; another sequence takes the freed low page ids; imported into another slot
    number of `dst` (src is dst: the same slot set; else the slots are created again); 40 more steps, crossing position 96, give the bits of K.reference"""
    st.create_slots(4, MAXSEQ, **src)
    st.prefill_slot(2, P["a"], chunk=24)
    tok, _ = _steps(st, [2], [F["a"]], [70], 5, [R["a"]], [0])
    img = st.export_slot(2, 75, release=True)
    if src:
        assert st.slot_pages()["per_slot"] == [0, 0, 0, 0] and st.slot_pages()["free"] == src["n_pages"]
    if dst is not src:
        st.create_slots(4, MAXSEQ, **dst)
    st.prefill_slot(0, P["b"], chunk=24)      # paged: the lowest page ids are this sequence's now
    assert st.import_slot(1, img) == 75
    if dst:
        ids, refs = st.slot_page_ids(1)
        n = -(-75 // dst["page_tokens"])
        assert all(i >= 0 for i in ids[:n]) and all(i < 0 for i in ids[n:]) and refs[:n] == [1] * n
        assert not set(ids[:n]) & set(st.slot_page_ids(0)[0][:2])
    _, pos = _steps(st, [1], tok, [75], 40, [R["a"]], [5])
    K.same(_slot_state(K, st, d, 1, pos[0]), R["a"][1])
    K.same(_slot_state(K, st, d, 0, 40), R["b40"])      # the bystander kept its bits
    return img


@pytest.mark.parametrize("kind,fp8", MODELS)
def test_round_trip_under_another_placement(kind, fp8):
    K, st, keep, d, P, F, R = _model(kind, fp8)
    images = [_round_trip(K, st, d, P, F, R, P32, P32), _round_trip(K, st, d, P, F, R, FLAT, P32), _round_trip(K, st, d, P, F, R, P64, FLAT)]
    assert images[0].tobytes() == images[1].tobytes() == images[2].tobytes()


# ---- 3: chunk edges ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,fp8", MODELS)
def test_chunks_of_1040_bytes_give_the_same_bytes_and_tokens(kind, fp8):
    """ranges that end inside rows and pages: tests 1 and 2 again with a staging half of 1040 bytes, against the images the default gives"""
    K, st, keep, d, P, F, R = _model(kind, fp8)
    whole = {n: _export_three_ways(K, st, d, P, F, "a", n)[0] for n in (70, 64)}
    trip = _round_trip(K, st, d, P, F, R, P32, P32)
    try:
        _chunk(st, 1040)
        for n in (70, 64):
            for img in _export_three_ways(K, st, d, P, F, "a", n):
                assert img.tobytes() == whole[n].tobytes(), n
        for src, dst in ((P32, P32), (FLAT, P32), (P64, FLAT)):
            assert _round_trip(K, st, d, P, F, R, src, dst).tobytes() == trip.tobytes()
    finally:
        _chunk(st, 0)


# ---- 4: several slots in one call ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,fp8", MODELS)
def test_several_slots_in_one_call(kind, fp8):
    K, st, keep, d, P, F, R = _model(kind, fp8)
    st.create_slots(4, MAXSEQ, **P32)
    st.prefill_slot(0, P["b"][:1]); st.prefill_slot(2, P["a"], chunk=24)
    st.set_slot_sampler(2, F["a"], temperature=0.7, top_k=5, top_p=0.9, presence_penalty=0.5, rng_seed=77)      # the set has samplers now: every image carries one
    slots, lens = [3, 0, 2], [0, 1, 70]
    many = st.export_slots(slots, lens)
    for s, n, img in zip(slots, lens, many):
        assert img.tobytes() == st.export_slot(s, n).tobytes(), (s, n)
        assert slot_image_info(img) == dict(seq_len=n, kv_fp8=bool(d.get("fp8")), has_sampler=True, geometry=slot_image_info(many[0])["geometry"])
        _image_equals_state(K, img, _slot_state(K, st, d, s, n), sampler=1)
    empty = _sections(many[0])      # seq_len 0: only linear-attention state and the sampler
    kinds = d["kinds"] if K is Gqa else ["mla"] * d["nL"]
    for li, kind_ in enumerate(kinds):
        assert (empty[2 * li].size > 0) == (kind_ == "la") and (empty[2 * li + 1].size > 0) == (kind_ == "la")
    words = (d["V"] + 31) // 32
    params = lambda t, k, p, pen: np.float32(t).tobytes() + np.int32(k).tobytes() + np.float32(p).tobytes() + np.float32(pen).tobytes()
    assert empty[-1].size == 32 + 4 * words and empty[-1][:16].tobytes() == params(0.0, 0, 1.0, 0.0) and not empty[-1][16:].any()      # no sampler was set on this slot: greedy
    smp = _sections(many[2])[-1]
    assert smp[:16].tobytes() == params(0.7, 5, 0.9, 0.5)
    seen, rng = st.slot_sampler_state(2)
    assert int(smp[16:24].view(np.uint64)[0]) == rng == 77 and smp[32:].tobytes() == seen.tobytes() and not smp[24:32].any()
    # one import call of the three, into other slots of another slot set, equals three single calls
    for together in (True, False):
        st.create_slots(4, MAXSEQ, **P64)
        st.prefill_slot(1, P["c"], chunk=24)      # what slot 1 held goes with the import
        if together:
            assert st.import_slots([1, 3, 0], many) == lens
        else:
            assert [st.import_slot(s, img) for s, img in zip([1, 3, 0], many)] == lens
        assert st.slot_pages()["per_slot"] == [2, 0, 0, 1]
        for s, n, img in zip([1, 3, 0], lens, many):
            assert st.export_slot(s, n).tobytes() == img.tobytes(), (together, s)
        K.same(_slot_state(K, st, d, 0, 70), R["a70"])
        seen2, rng2 = st.slot_sampler_state(0)
        assert rng2 == 77 and np.array_equal(seen2, seen)


# ---- 5: fork ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,fp8", MODELS)
def test_export_and_import_beside_shared_pages(kind, fp8):
    K, st, keep, d, P, F, R = _model(kind, fp8)
    st.create_slots(4, MAXSEQ, **P32)
    st.prefill_slot(1, P["b"], chunk=24)
    other = st.export_slot(1, 40, release=True)
    st.prefill_slot(2, P["a"], chunk=24)
    st.fork_slot(2, [0, 3], 70)      # the boundary copies are still queued when the export starts
    before = _tables(st, 4)
    assert before[0][0][1][:3] == [3, 3, 1] and before[0][2][1][:3] == [3, 3, 1]
    img = st.export_slot(0, 70)
    assert _tables(st, 4) == before      # no copy-on-write, no reference moved
    assert img.tobytes() == st.export_slot(2, 70).tobytes()
    _image_equals_state(K, img, R["a70"])
    assert st.import_slot(3, other) == 40      # slot 3 drops its references: the shared pages go from 3 holders to 2
    ids, refs = st.slot_page_ids(3)
    assert refs == [1, 1, 0, 0] and not set(ids[:2]) & set(st.slot_page_ids(0)[0][:3])
    assert st.slot_page_ids(0)[1][:3] == [2, 2, 1] and st.slot_page_ids(2)[1][:3] == [2, 2, 1]
    K.same(_slot_state(K, st, d, 3, 40), R["b40"])
    K.same(_slot_state(K, st, d, 0, 70), R["a70"])
    K.same(_slot_state(K, st, d, 2, 70), R["a70"])
    _steps(st, [2, 0, 3], [F["a"], F["a"], F["b"]], [70, 70, 40], 3, [R["a"], R["a"], R["b"]], [0, 0, 0])      # slot 2's next steps match its reference, and so do the others'


# ---- 6: pool exhaustion ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,fp8", MODELS)
def test_an_import_that_does_not_fit_changes_nothing(kind, fp8):
    K, st, keep, d, P, F, R = _model(kind, fp8)
    st.create_slots(4, MAXSEQ, page_tokens=PT, n_pages=6)
    st.prefill_slot(0, P["a"], chunk=24); st.prefill_slot(1, P["b"], chunk=24); st.prefill_slot(2, P["c"][:20])
    img = st.export_slot(0, 70)
    before = _tables(st, 4)
    assert before[1]["free"] == 0 and before[1]["per_slot"] == [3, 2, 1, 0]
    state = _slot_state(K, st, d, 1, 40)
    # three pages needed, none free, two come back with the target: one short
    _state_error(lambda: st.import_slot(1, img), "pages", "3 pages", "2 of 6")
    assert _tables(st, 4) == before
    K.same(_slot_state(K, st, d, 1, 40), state); K.same(state, R["b40"])
    _steps(st, [1], [F["b"]], [40], 2, [R["b"]], [0])      # positions 40 and 41 lie in its second page: no page needed
    st.trim_slot(2, 0)      # one page free: alone it would not do, with the target's own two it does
    assert st.slot_pages()["free"] == 1
    assert st.import_slot(1, img) == 70
    assert st.slot_pages()["per_slot"] == [3, 3, 0, 0] and st.slot_pages()["free"] == 0 and st.slot_page_ids(1)[1] == [1, 1, 1, 0]
    K.same(_slot_state(K, st, d, 1, 70), R["a70"])
    _steps(st, [0, 1], [F["a"]] * 2, [70, 70], 3, [R["a"], R["a"]], [0, 0])


# ---- 7: the sampler travels with the slot ----------------------------------------------------------------------------------------------------------------
SAMPLER = dict(temperature=0.9, top_k=20, top_p=0.9, presence_penalty=0.6, rng_seeds=12345)


@pytest.mark.parametrize("kind,fp8", MODELS)
def test_a_sampled_generation_cut_by_a_swap(kind, fp8):
    K, st, keep, d, P, F, R = _model(kind, fp8)
    st.create_slots(4, MAXSEQ, **P32)
    st.prefill_slot(2, P["b"], chunk=24)
    truth = st.generate_multi([2], [F["b"]], [40], 24, **SAMPLER)[0]      # the uncut run
    final = st.slot_sampler_state(2)
    assert len(truth) == 24
    st.create_slots(4, MAXSEQ, **P32)
    st.prefill_slot(2, P["b"], chunk=24)
    assert st.generate_multi([2], [F["b"]], [40], 10, **SAMPLER)[0] == truth[:10]
    img = st.export_slot(2, 50, release=True)
    assert slot_image_info(img)["has_sampler"] and st.slot_pages()["free"] == P32["n_pages"]
    st.set_slot_sampler(0, 1, temperature=0.3, rng_seed=5)      # the target's own sampler goes with what it held
    assert st.import_slot(0, img) == 50
    got, tok = [], truth[9]
    for k in range(14):
        tok = st.step_multi_sample([0], [tok], [50 + k])[0]
        got.append(tok)
    assert got == truth[10:]
    seen, rng = st.slot_sampler_state(0)
    assert rng == final[1] and np.array_equal(seen, final[0])


@pytest.mark.parametrize("kind,fp8", [MODELS[0], MODELS[3]])
def test_an_image_without_a_sampler_leaves_the_slot_greedy(kind, fp8):
    K, st, keep, d, P, F, R = _model(kind, fp8)
    st.create_slots(4, MAXSEQ, **P32)      # no sampler was ever set on these
    st.prefill_slot(2, P["b"], chunk=24)
    img = st.export_slot(2, 40)
    assert not slot_image_info(img)["has_sampler"]
    st.create_slots(4, MAXSEQ, **FLAT)
    st.set_slot_sampler(1, F["b"], temperature=1.0, top_k=0, presence_penalty=1.0, rng_seed=9)
    assert st.import_slot(1, img) == 40
    seen, rng = st.slot_sampler_state(1)
    assert rng == 0 and not seen.any()
    tok = F["b"]
    for k in range(6):      # its sampler draws the greedy ids
        tok = st.step_multi_sample([1], [tok], [40 + k])[0]
        assert tok == R["b"][0][k][1], k


# ---- 8: refusals, each changing nothing ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,cfg,other", [(Gqa, dict(seed=3, hd=64, nh=4), dict(seed=3, hd=128, nh=8)), (Mla, mla.CFGS[0], mla.CFGS[2])])
def test_refusals_change_nothing(K, cfg, other):
    st, keep, d = K.build(False, kv_max=128, **cfg)
    rng = np.random.default_rng(5)
    prompt, first = _toks(rng, d, 40), _toks(rng, d, 1)[0]
    st.create_slots(3, MAXSEQ, page_tokens=PT, n_pages=8)
    st.prefill_slot(0, prompt, chunk=24)
    fp16 = st.export_slot(0, 40)
    st2, keep2, d2 = K.build(True, kv_max=128, **other)
    st2.create_slots(1, MAXSEQ)
    alien = st2.export_slot(0, 40)
    del st2, keep2
    st.set_kv_dtype(True); d["fp8"] = True
    st.create_slots(3, MAXSEQ, page_tokens=PT, n_pages=8)
    long_ = st.export_slot(0, 100)      # an empty slot: its rows export as zeros; only the header matters below
    st.create_slots(3, 64, page_tokens=PT, n_pages=8)
    st.prefill_slot(0, prompt, chunk=24); st.prefill_slot(1, prompt[:20])
    good = st.export_slot(0, 40)
    st.set_slot_sampler(1, first, temperature=0.5, rng_seed=3)      # the set has samplers from here on: this image carries one
    hot = []
    for t in (-1.0, float("nan")):      # a temperature the sampler's setter refuses
        img = st.export_slot(0, 40)
        _sections(img)[-1][:4] = np.frombuffer(np.float32(t).tobytes(), np.uint8)
        hot.append(img)

    def snapshot():
        arrays = [x for s, n in ((0, 40), (1, 20)) for pair in _pairs(K, _slot_state(K, st, d, s, n)) for x in pair]
        return _tables(st, 3), arrays + [st.slot_sampler_state(s)[0] for s in range(3)], [st.slot_sampler_state(s)[1] for s in range(3)]

    def same(a, b):
        assert a[0] == b[0] and a[2] == b[2] and len(a[1]) == len(b[1])
        assert all(np.array_equal(x, y) for x, y in zip(a[1], b[1]))

    before = snapshot()
    flipped = good.copy(); flipped[1] ^= 0x40
    version = good.copy(); version[4] = 2
    for bad, word in ((good[:-16], "total_bytes"), (flipped, "magic"), (version, "version"), (fp16, "KV element type"), (alien, "geometry"), (long_, "seq_len"),
                      (hot[0], "temperature"), (hot[1], "temperature")):
        with pytest.raises(ValueError, match="row 0") as e:
            st.import_slot(1, bad)
        assert word in str(e.value), (word, str(e.value))
    with pytest.raises(ValueError, match="row 1.*named twice"):
        st.import_slots([1, 1], [good, good])
    with pytest.raises(ValueError, match="row 1.*named twice"):
        st.export_slots([0, 0], [40, 40])
    with pytest.raises(ValueError, match="out of range"):
        st.import_slot(3, good)
    with pytest.raises(ValueError, match="seq_len"):
        st.export_slot(0, 65)
    import ctypes as C
    n = C.c_size_t(good.size - 16)      # a wrong byte count on the way out
    with pytest.raises(ValueError, match="row 0: image_bytes"):
        from krasis_amd._lib import check
        check(st._lib.kr_decode_slots_export(st._h, 1, (C.c_int32 * 1)(0), (C.c_int32 * 1)(40), (C.c_void_p * 1)(good.ctypes.data), C.byref(n), 0))
    for v in (0, 1000, 1032, -16):
        with pytest.raises(ValueError, match="slot_swap_chunk_bytes"):
            st.set_option("slot_swap_chunk_bytes", v)
    same(snapshot(), before)
    st.verify_multi([0], [[first, first]], [40])      # between a verify over slots and its commit nothing else runs on them
    _state_error(lambda: st.import_slot(1, good), "pending")
    _state_error(lambda: st.export_slot(0, 40), "pending")
    st.commit_multi([1])
    assert st.import_slot(2, st.export_slot(0, 41)) == 41 and st.import_slot(1, good) == 40      # and after the commit both run


# ---- 9: preempt and resume -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,fp8", MODELS)
def test_preempt_and_resume(kind, fp8):
    """a pool of five pages holds two sequences but not three: A is swapped out to let C in, and comes back when C has finished"""
    K, st, keep, d, P, F, R = _model(kind, fp8)
    st.create_slots(3, MAXSEQ, page_tokens=PT, n_pages=5)
    st.prefill_slot(0, P["a40"], chunk=24); st.prefill_slot(1, P["b"], chunk=24)
    (ta, tb), _ = _steps(st, [0, 1], [F["a40"], F["b"]], [40, 40], 10, [R["a40"], R["b"]], [0, 0])
    _state_error(lambda: st.prefill_slot(2, P["c"], chunk=40), "pages")      # no room for the newcomer
    image_a = st.export_slot(0, 50, release=True)      # A leaves the device
    st.prefill_slot(2, P["c"], chunk=40)
    (tb, tc), _ = _steps(st, [1, 2], [tb, F["c"]], [50, 40], 5, [R["b"], R["c"]], [10, 0])
    _steps(st, [2], [tc], [45], 15, [R["c"]], [5])      # C decodes to its end
    K.same(_slot_state(K, st, d, 2, 60), R["c"][1])
    st.trim_slot(2, 0)
    assert st.import_slot(2, image_a) == 50      # A comes back, into another slot, and goes on beside B
    (ta, tb), _ = _steps(st, [2, 1], [ta, tb], [50, 55], 5, [R["a40"], R["b"]], [10, 15])      # B's last steps
    _steps(st, [2], [ta], [55], 15, [R["a40"]], [15])      # A finishes, across position 64: a third page
    K.same(_slot_state(K, st, d, 2, 70), R["a40"][1])
    K.same(_slot_state(K, st, d, 1, 60), R["b"][1])
    assert _pages(70) == 3 and st.slot_pages()["per_slot"] == [0, 2, 3] and st.slot_pages()["free"] == 0
