"""Paged and forked slots at serving sizes (docs/design/21-paged-slots.md, 22-slot-fork.md): rows of thousands of positions behind page tables of hundreds of
entries, pages of 256 tokens, batches across the 32-row switch, hundreds of tokens mapped by one call, forks that share whole 256-token pages, and the LDS
budget of the paged GQA launch.  The reference is never the paged path: it is the single-sequence path (decode_step, prefill, get_decode_state through the
helpers of the neighbouring suites) and, where a call sequence is replayed, flat slots of the same store.  Every assertion is on ids and on u32 / stored-row
bit patterns.

Long rows do not come from an 8000-token prompt pass: the store is given a random state of the wanted length (set_decode_state), save_slot copies it into
the slot, and the reference is decode_step on the store from that same state."""
import functools

import numpy as np
import pytest

from oracle import oracle as O
from tests.test_multi_paged_gpu import Gqa, Mla, _prefill_then_steps, _slot_state, _toks

pytestmark = pytest.mark.gpu
F = np.float32
U = np.uint32


# ---- random states of a store, one per slot --------------------------------------------------------------------------------------------------------------
def _rows(rng, shape, fp8, codes=False):
    """stored rows: FP16 bits of standard_normal * 0.5; E4M3 the same values rounded, or (codes) every code but the two NaNs, as tests/test_decode_gpu.py makes them"""
    if not fp8:
        return O.f32_to_f16_bits((rng.standard_normal(shape) * 0.5).astype(F))
    if codes:
        b = rng.integers(0, 256, shape).astype(np.uint8)
        b[(b & 0x7F) == 0x7F] = 0x3C
        return b
    return O.f32_to_e4m3((rng.standard_normal(shape) * 0.5).astype(F))


def _variants(base, n):
    """n different states from one: every array rolled by another amount along its first axis -- no two slots hold the same row at the same position"""
    return [[None if a is None else np.ascontiguousarray(np.roll(a, 997 * i + 13 * (i > 0), axis=0)) for a in base] for i in range(n)]


def _gqa_states(K, d, rng, n):
    """hybrid / GQA-only store: per layer K rows (values that spread the softmax), V rows (E4M3: every finite code), conv and recurrent state"""
    fp8, w = bool(d.get("fp8")), d["nkv"] * d["hd"]
    k, v, conv, recur = [], [], [], []
    for kind in d["kinds"]:
        gqa = kind != "la"
        k.append(_rows(rng, (d["kv_max"], w), fp8) if gqa else None)
        v.append(_rows(rng, (d["kv_max"], w), fp8, codes=True) if gqa else None)
        conv.append(None if gqa else ((rng.random(d["conv_dim"] * 4) - 0.5) * 0.2).astype(F))
        recur.append(None if gqa else ((rng.random(d["nv"] * d["dk"] * d["dv"]) - 0.5) * 0.02).astype(F))
    return list(zip(_variants(k, n), _variants(v, n), _variants(conv, n), _variants(recur, n)))


def _mla_states(K, d, rng, n):
    """MLA store: latent and rope-key rows of every layer.  The latent rows are keys and values at once, so E4M3 rows are rounded normal values, not raw codes:
    codes up to 448 would leave one position with all of the softmax and a misplaced page elsewhere unseen"""
    ck = [_rows(rng, (d["kv_max"], d["klr"]), d["fp8"]) for _ in range(d["nL"])]
    kp = [_rows(rng, (d["kv_max"], d["rd"]), d["fp8"]) for _ in range(d["nL"])]
    return list(zip(_variants(ck, n), _variants(kp, n)))


def _inject(K, st, d, state):
    z = lambda xs: [x.ctypes.data if x is not None else 0 for x in xs]
    if K is Mla:
        n = d["nL"]
        st.set_decode_state(0, d["kv_max"], [0] * n, [0] * n, [0] * n, [0] * n, z(state[0]), z(state[1]))
    else:
        st.set_decode_state(0, d["kv_max"], z(state[0]), z(state[1]), z(state[2]), z(state[3]))


def _states(K, d, rng, n):
    return (_mla_states if K is Mla else _gqa_states)(K, d, rng, n)


def _decode_reference(K, st, d, state, first, pos, n_steps):
    """decode_step on the store from the injected state, the greedy continuation of `first` at position pos: per step (logits bits, id), then the state snapshot"""
    _inject(K, st, d, state)
    out, tok = [], first
    for k in range(n_steps):
        st.decode_step(tok, pos + k)
        out.append((st.read_logits().view(U).copy(), st.last_token()))
        tok = out[-1][1]
    return out, K.snap(st, d, pos + n_steps)


def _pages(n, pt):
    return (n + pt - 1) // pt


# ---- 1, 2: long rows ---------------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _long_model(kind, key):
    """the store of one geometry, three random states and their single-sequence references: built once, shared by both page sizes, never changed"""
    if kind == "gqa":
        hd, nh, fp8 = key
        K, lens = Gqa, (700, 2500, 8300)
        st, keep, d = Gqa.build(fp8, seed=3, hd=hd, nh=nh, kv_max=8448)
    else:
        K, lens = Mla, (300, 4100, 8400)
        cfg, fp8 = [(dict(nh=11), False), (dict(klr=256, seed=4), True), (dict(seed=6), True)][key]
        st, keep, d = Mla.build(fp8, kv_max=8600, **cfg)
    rng = np.random.default_rng(77)
    states = _states(K, d, rng, 3)
    firsts = _toks(rng, d, 3)
    refs = [_decode_reference(K, st, d, s, f, n, 2) for s, f, n in zip(states, firsts, lens)]
    return K, st, keep, d, states, firsts, lens, refs


def _long_rows(kind, key, page_tokens):
    K, st, keep, d, states, firsts, lens, refs = _long_model(kind, key)
    pt = page_tokens
    slots, spare = [2, 0, 3], 1                                    # rows in scrambled slot order
    n_pages = sum(_pages(n + 2, pt) for n in lens)
    st.create_slots(4, max(lens) + 40, page_tokens=pt, n_pages=n_pages)
    _inject(K, st, d, states[0]); st.save_slot(slots[0], lens[0])
    st.save_slot(spare, 100)                                       # pages between the first and the second row ...
    _inject(K, st, d, states[1]); st.save_slot(slots[1], lens[1])
    st.trim_slot(spare, 0)                                         # ... that come back as a hole: lowest free id first hands it to the longest row
    _inject(K, st, d, states[2]); st.save_slot(slots[2], lens[2])
    ids = st.slot_page_ids(slots[2])[0]
    used = ids[:_pages(lens[2], pt)]
    assert min(used) >= 0 and all(i == -1 for i in ids[len(used):])
    assert len(set(np.diff(used).tolist())) > 1, "the longest row's pages are an arithmetic progression"
    assert used[0] == _pages(lens[0], pt) and used[_pages(100, pt)] == _pages(lens[0], pt) + _pages(100, pt) + _pages(lens[1], pt)
    toks, pos = list(firsts), list(lens)
    for k in range(2):
        got, lg = st.step_multi(slots, toks, pos, logits=True)
        for i, (ref, _) in enumerate(refs):
            assert np.array_equal(lg[i].view(U), ref[k][0]), ("logits", k, i)
            assert got[i] == ref[k][1], ("id", k, i)
        toks = got; pos = [p + 1 for p in pos]
    pages = st.slot_pages()
    assert [pages["per_slot"][s] for s in slots] == [_pages(p, pt) for p in pos] and pages["free"] == 0
    for i, (_, snap) in enumerate(refs):
        K.same(_slot_state(K, st, d, slots[i], pos[i]), snap)


@pytest.mark.parametrize("page_tokens", [32, 256])
@pytest.mark.parametrize("hd,nh,fp8", [(256, 16, False), (128, 8, True), (64, 4, False)])
def test_long_gqa_rows(hd, nh, fp8, page_tokens):
    """rows of 700, 2500 and 8300 positions in one step: 260 table entries at page_tokens 32 take the second round of the kernel's table load into LDS, the
    softmax tiles of 1024 positions cross page edges, pages of 256 give in-page offsets up to 255; the longest row's pages are not contiguous"""
    _long_rows("gqa", (hd, nh, fp8), page_tokens)


@pytest.mark.parametrize("page_tokens", [32, 256])
@pytest.mark.parametrize("cfg", [0, 1, 2])
def test_long_mla_rows(cfg, page_tokens):
    """the three stores of test_multi_mla_gpu.py::test_long_caches (nh 11 FP16, klr 256 E4M3, default E4M3), rows of 300, 4100 and 8400 positions: a page of
    256 tokens is eight stages of the kernel, 4100 and 8400 end inside one at rows 4 and 208, so num_records cuts a page between two of its stages and the
    stage prefetched past the end lies in a mapped page"""
    _long_rows("mla", cfg, page_tokens)


# ---- 3: batch widths -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [Gqa, Mla])
def test_batch_widths_and_row_order(K):
    """B = 31, 32, 33, 64 and the 64 rows permuted, page_tokens 32, prompts of 1 .. 40 tokens so that some rows step across a page edge: the 32-row switch to
    the matrix-core absorption and w_vc launches runs with a page table.  Mirrors test_batch_sizes_and_row_order of the flat suites"""
    st, keep, d = K.build(kv_max=48)
    rng = np.random.default_rng(9)
    n_seq, pt = 64, 32
    prompts = [_toks(rng, d, int(rng.integers(1, 41))) for _ in range(n_seq)]
    prompts[0], prompts[1], prompts[2] = prompts[0][:1] * 31, prompts[1][:1] * 32, prompts[2][:1] * 33      # the step's own row is the last of a page, the first of the next, the second
    firsts = _toks(rng, d, n_seq)
    refs = [K.reference(st, d, p, f, 1)[0][0] for p, f in zip(prompts, firsts)]
    perm = [int(x) for x in rng.permutation(64)]
    groups, base = [], 0
    for B in (31, 32, 33, 64):
        groups.append((list(range(B)), list(range(base, base + B)))); base += B
    groups.append((perm, list(range(base, base + 64)))); base += 64
    n_pages = sum(_pages(len(prompts[q]) + 1, pt) for seqs, _ in groups for q in seqs)
    st.create_slots(base, 48, page_tokens=pt, n_pages=n_pages)
    per_seq = [[] for _ in range(n_seq)]
    for seqs, slots in groups:
        for q, s in zip(seqs, slots):
            per_seq[q].append(s)
    for p, slots in zip(prompts, per_seq):
        K.start(st, d, p)
        for s in slots:
            st.save_slot(s, len(p))
    for seqs, slots in groups:
        ids, lg = st.step_multi(slots, [firsts[q] for q in seqs], [len(prompts[q]) for q in seqs], logits=True)
        for r, q in enumerate(seqs):
            assert np.array_equal(lg[r].view(U), refs[q][0]), (len(seqs), r, q)
            assert ids[r] == refs[q][1], (len(seqs), r, q)
    assert st.slot_pages()["free"] == 0


# ---- 4: many pages in one call ---------------------------------------------------------------------------------------------------------------------------
def _extend_many(K, st, d, paged, prompts, page_tokens):
    """one extend_multi with runs of 300, 1 and 130 tokens from positions 20, 63 and 0 -> everything it produced"""
    starts = (20, 63, 0)
    st.create_slots(4, 340, **(dict(page_tokens=page_tokens, n_pages=sum(_pages(len(p), page_tokens) for p in prompts)) if paged else {}))
    slots = [3, 0, 2]
    for s, p, n in zip(slots, prompts, starts):
        if n:
            st.prefill_slot(s, p[:n], chunk=24)
    ids, lg = st.extend_multi(slots, [p[n:] for p, n in zip(prompts, starts)], list(starts), logits=True)
    if paged:
        pages = st.slot_pages()
        assert [pages["per_slot"][s] for s in slots] == [_pages(len(p), page_tokens) for p in prompts] and pages["free"] == 0
    return ids, lg.view(U).copy(), [_slot_state(K, st, d, s, len(p)) for s, p in zip(slots, prompts)]


@pytest.mark.parametrize("page_tokens", [32, 64])
@pytest.mark.parametrize("K", [Gqa, Mla])
def test_many_pages_mapped_by_one_call(K, page_tokens):
    """a run of 300 tokens maps ten pages of 32 in one reservation and one zero launch, next to a run of one token at a page's last row and a run into a fresh slot"""
    st, keep, d = K.build(kv_max=352)
    rng = np.random.default_rng(91)
    prompts = [_toks(rng, d, n) for n in (320, 64, 130)]
    refs = []
    for p in prompts:
        K.start(st, d, p)
        refs.append((st.read_logits().view(U).copy(), st.last_token(), K.snap(st, d, len(p))))
    got = _extend_many(K, st, d, True, prompts, page_tokens)
    flat = _extend_many(K, st, d, False, prompts, page_tokens)
    for i, (lg, tok, snap) in enumerate(refs):
        assert np.array_equal(got[1][i], lg) and got[0][i] == tok, i
        K.same(got[2][i], snap)
        K.same(flat[2][i], got[2][i])
    assert got[0] == flat[0] and np.array_equal(got[1], flat[1])


# ---- 5: fork at length -----------------------------------------------------------------------------------------------------------------------------------
N_FORK, REWIND, N_NEW = 2500, 1000, 20
SRC, DSTS = 4, [1, 3, 0]


def _fork_run(K, st, d, paged, state, firsts, new):
    """the call sequence of the fork test on paged or flat slots -> everything it produced"""
    pt, n_pages = 256, 15                                          # ten pages of the source, three boundary copies, one private copy, one to spare
    st.create_slots(5, 2600, **(dict(page_tokens=pt, n_pages=n_pages) if paged else {}))
    _inject(K, st, d, state); st.save_slot(SRC, N_FORK)
    full = N_FORK // pt                                            # nine whole pages; the boundary page holds 196 rows
    if paged:
        src_ids = st.slot_page_ids(SRC)
        assert src_ids[0][:full + 1] == list(range(full + 1)) and src_ids[1][:full + 1] == [1] * (full + 1)
    st.fork_slot(SRC, DSTS, N_FORK)
    if paged:
        tables = [st.slot_page_ids(s) for s in [SRC] + DSTS]
        for ids, refc in tables:
            assert ids[:full] == list(range(full)) and refc[:full] == [4] * full and ids[full + 1:] == [-1] * (len(ids) - full - 1)
        assert [ids[full] for ids, _ in tables] == [full, full + 1, full + 2, full + 3] and all(refc[full] == 1 for _, refc in tables)
        assert st.slot_pages()["free"] == n_pages - (full + 1) - 3
    out = []
    toks, pos = list(firsts[:3]), [N_FORK] * 3
    for k in range(3):                                             # every destination with its own first token
        ids, lg = st.step_multi(DSTS, toks, pos, logits=True)
        out.append((list(ids), lg.view(U).copy()))
        toks = ids; pos = [p + 1 for p in pos]
    out.append(st.extend_multi([DSTS[0]], [new], [REWIND], logits=True))      # a write below the fork point: positions [1000, 1020), all in page 3
    out[-1] = (list(out[-1][0]), out[-1][1].view(U).copy())
    if paged:
        ids, refc = st.slot_page_ids(DSTS[0])
        hit = REWIND // pt
        assert ids[hit] == full + 4 and refc[hit] == 1             # a private copy of the whole 256-token page, on the lowest free id
        assert ids[:hit] == list(range(hit)) and ids[hit + 1:full] == list(range(hit + 1, full)) and ids[full] == full + 1
        assert [r for j, r in enumerate(refc[:full]) if j != hit] == [4] * (full - 1)
        for s in [SRC] + DSTS[1:]:
            ids, refc = st.slot_page_ids(s)
            assert ids[:full] == list(range(full)) and refc[hit] == 3 and [r for j, r in enumerate(refc[:full]) if j != hit] == [4] * (full - 1)
        assert st.slot_pages()["free"] == n_pages - (full + 1) - 3 - 1
    out.append(st.step_multi([SRC, DSTS[0]], [firsts[3], firsts[4]], [N_FORK, REWIND + N_NEW], logits=True))
    out[-1] = (list(out[-1][0]), out[-1][1].view(U).copy())
    states = [_slot_state(K, st, d, SRC, N_FORK + 1), _slot_state(K, st, d, DSTS[0], REWIND + N_NEW + 1), _slot_state(K, st, d, DSTS[1], N_FORK + 3)]
    return out, states


@pytest.mark.parametrize("K", [Gqa, Mla])
def test_fork_at_length(K):
    """page_tokens 256: a 2500-position source forked to three destinations shares nine whole pages and gives each a boundary page of 196 copied and 60 zeroed
    rows (pages of 256 KiB in the GQA-only store: head_dim 256, two KV heads, FP16); three steps each, then one destination is rewound to position 1000"""
    if K is Gqa:
        st, keep, d = Gqa.build(False, seed=3, hd=256, nh=16, kv_max=2600, kinds=["gqa", "gqa"])
    else:
        st, keep, d = Mla.build(True, kv_max=2600)
    rng = np.random.default_rng(92)
    state = _states(K, d, rng, 1)[0]
    firsts, new = _toks(rng, d, 5), _toks(rng, d, N_NEW)
    # the single-sequence reference of each slot's own history
    dst_refs = [_decode_reference(K, st, d, state, f, N_FORK, 3) for f in firsts[:3]]
    src_ref = _decode_reference(K, st, d, state, firsts[3], N_FORK, 1)
    _inject(K, st, d, state)
    st.prefill(new, REWIND)
    rewind_ref = (st.read_logits().view(U).copy(), st.last_token())
    st.decode_step(firsts[4], REWIND + N_NEW)
    rewound_ref = (st.read_logits().view(U).copy(), st.last_token(), K.snap(st, d, REWIND + N_NEW + 1))
    got, states = _fork_run(K, st, d, True, state, firsts, new)
    flat, flat_states = _fork_run(K, st, d, False, state, firsts, new)
    for k in range(3):
        for i, (ref, _) in enumerate(dst_refs):
            assert np.array_equal(got[k][1][i], ref[k][0]) and got[k][0][i] == ref[k][1], (k, i)
    assert np.array_equal(got[3][1][0], rewind_ref[0]) and got[3][0][0] == rewind_ref[1]
    assert np.array_equal(got[4][1][0], src_ref[0][0][0]) and got[4][0][0] == src_ref[0][0][1]
    assert np.array_equal(got[4][1][1], rewound_ref[0]) and got[4][0][1] == rewound_ref[1]
    K.same(states[0], src_ref[1]); K.same(states[1], rewound_ref[2]); K.same(states[2], dst_refs[1][1])
    assert len(got) == len(flat)
    for (ids, lg), (fids, flg) in zip(got, flat):
        assert ids == fids and np.array_equal(lg, flg)
    for a, b in zip(states, flat_states):
        K.same(a, b)


# ---- 6: the LDS budget of the paged GQA launch -----------------------------------------------------------------------------------------------------------
def _table_limit(hd, nh, nkv=2):
    """kr_multi_gqa_attn_kernel keeps, in 64 KiB of dynamic LDS, G = nh / nkv query rows of hd floats, four softmax tiles of 1024 floats, a P.V tile of G x 64
    floats and the slot's table row: the entries that fit beside the rest (docs/design/21-paged-slots.md, "Contract")"""
    G = nh // nkv
    return (64 * 1024 - (G * hd + 4 * 1024 + G * 64) * 4) // 4


@pytest.mark.parametrize("hd,nh", [(256, 16), (64, 4)])
def test_table_one_entry_over_the_lds_budget_is_refused_at_creation(hd, nh):
    """before the check at creation such a slot set was created, and every batched call failed inside the pass ("unsupported GQA geometry"), at the first GQA
    layer: with its pages mapped and the conv and recurrent state of the linear-attention layer in front already advanced"""
    st, keep, d = Gqa.build(seed=3, hd=hd, nh=nh, kv_max=128)
    limit = _table_limit(hd, nh)
    assert limit == {(256, 16): 9728, (64, 4): 12032}[(hd, nh)]
    rng = np.random.default_rng(93)
    prompt, first = _toks(rng, d, 40), _toks(rng, d, 1)[0]
    ref = Gqa.reference(st, d, prompt, first, 2)
    st.create_slots(3, 100, page_tokens=32, n_pages=6)
    st.prefill_slot(1, prompt, chunk=24)
    before = st.slot_pages()
    for max_seq in (limit * 32 + 1, limit * 32 + 32, limit * 64):
        with pytest.raises(ValueError) as e:
            st.create_slots(3, max_seq, page_tokens=32, n_pages=6)
        for needle in ("max_seq %d" % max_seq, "page_tokens 32", "layer 1", "at most %d entries" % limit):
            assert needle in str(e.value), (needle, str(e.value))
    assert st.slot_pages() == before                                # the earlier slot set is in place ...
    toks, pos = [first], [40]
    for k in range(2):                                              # ... and steps as the sequence alone
        ids, lg = st.step_multi([1], toks, pos, logits=True)
        assert np.array_equal(lg[0].view(U), ref[0][k][0]) and ids[0] == ref[0][k][1], k
        toks = ids; pos = [p + 1 for p in pos]
    Gqa.same(_slot_state(Gqa, st, d, 1, 42), ref[1])


@pytest.mark.parametrize("hd,nh", [(256, 16), (64, 4)])
def test_table_exactly_at_the_lds_budget_steps(hd, nh):
    """the largest capacity that is created asks the attention launch for exactly 64 KiB of LDS: prompts of 0, 31 and 70 tokens, six steps across positions 32 and 64"""
    st, keep, d = Gqa.build(seed=3, hd=hd, nh=nh, kv_max=128)
    _prefill_then_steps(Gqa, st, d, n_pages=6, n_steps=6, max_seq=_table_limit(hd, nh) * 32)
    assert len(st.slot_page_ids(0)[0]) == _table_limit(hd, nh)
