"""The "multi_attn_fast_paged" option (docs/design/23-multi-attn-fast-paged.md): split-KV flash-decode of the batched decode over PAGED slots.  With it set,
over paged slots of max_seq > 1024, row i of every batched call is BIT-IDENTICAL to the same call on flat slots of the same n_slots and max_seq under
"multi_attn_fast", and so to decode_step under set_attention_mode(True) on that sequence alone -- for any page size, any placement of the pages in the pool,
pages shared by fork, any batch composition, FP16 and E4M3, head_dim 64 / 128 / 256.  Shorter paged slots keep the exact paged step; flat slots behave as under
"multi_attn_fast".

The reference is never the paged flash path: it is the single-sequence fast step (the references of tests/test_multi_attn_fast_gpu.py, computed once and
shared), the same call sequence on flat slots under "multi_attn_fast", or, for the stated tolerance, the option-off paged step.  Every comparison but that
one is on ids and u32 / stored-row bit patterns."""
import functools

import numpy as np
import pytest

from tests import test_multi_attn_fast_gpu as FL
from tests import test_multi_paged_scale_gpu as SC
from tests.test_multi_attn_fast_gpu import KV_MAX, LENS, MODELS, N_STEPS, _fast_reference, _fill_slots, _get, _start
from tests.test_multi_paged_gpu import Gqa, _slot_state, _state_error, _toks
from tests.test_speculative_gpu import _same, _snap

pytestmark = pytest.mark.gpu
F = np.float32
U = np.uint32
OPT = "multi_attn_fast_paged"
SLOT_SEQ = 1200
LONG = LENS.index(1150)

_stores = []                                     # stores this file built itself (the flat suite's are reached through FL._built)


@pytest.fixture(autouse=True)
def options_off_afterwards():
    yield
    for st in [FL._model(*key)[0] for key in MODELS if key in FL._built] + _stores:
        st.set_option(OPT, 0); st.set_option("multi_attn_fast", 0); st.set_attention_mode(False)


def _pages(n, pt):
    return (n + pt - 1) // pt


def _bits(lg):
    return lg.view(U).copy()


# ---- 1: rows equal the single-sequence fast step ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("page_tokens", [32, 64, 256])
@pytest.mark.parametrize("hd,nh,fp8", MODELS)
def test_row_equals_single_sequence_fast_step(hd, nh, fp8, page_tokens):
    """page_tokens 32: a tile of 64 positions spans two pages and a chunk four; 64: a tile is a page; 256: a chunk lies inside a page and in-page offsets reach
    255.  Rows in scrambled slot order; the longest row's pages are not contiguous: a spare slot saved between the fills leaves a hole that row takes first"""
    st, _, d, prompts, firsts, refs = _get(hd, nh, fp8)
    pt = page_tokens
    slots, spare = [4, 0, 6, 2, 7, 1, 5], 3
    st.create_slots(8, SLOT_SEQ, page_tokens=pt, n_pages=sum(_pages(n + N_STEPS, pt) for n in LENS) + 2)
    _fill_slots(st, d, prompts[:5], [[s] for s in slots[:5]])
    st.save_slot(spare, 100)                                                # pages between the short rows and the 700-position row ...
    _fill_slots(st, d, prompts[5:6], [[slots[5]]])
    st.trim_slot(spare, 0)                                                  # ... come back as a hole: lowest free id first hands it to the longest row
    _fill_slots(st, d, prompts[6:], [[slots[6]]])
    used = st.slot_page_ids(slots[LONG])[0][:_pages(LENS[LONG], pt)]
    assert min(used) >= 0 and len(set(np.diff(used).tolist())) > 1, ("the longest row's pages are an arithmetic progression", used)
    st.set_option(OPT, 1)
    toks, pos = list(firsts), [len(p) for p in prompts]
    for k in range(N_STEPS):
        ids, lg = st.step_multi(slots, toks, pos, logits=True)
        for i, (ref, _) in enumerate(refs):
            assert np.array_equal(lg[i].view(U), ref[k][0]), ("logits", k, LENS[i])
            assert ids[i] == ref[k][1], ("id", k, LENS[i])
        toks = [ref[k][1] for ref, _ in refs]; pos = [p + 1 for p in pos]
    st.set_option(OPT, 0)
    for i, (_, snap) in enumerate(refs):
        _same(_slot_state(Gqa, st, d, slots[i], pos[i]), snap)


# ---- 2: the rest of a page does not leak in -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hd,nh,fp8", [(256, 16, False), (128, 8, True)])
def test_rows_past_the_length_do_not_leak_in(hd, nh, fp8):
    """pages returned dirty by a trim and handed out again; slots whose last pages hold the rejected rows of a verify that kept nothing: 5 drafted tokens from
    position 127 (they cross the chunk and page edge at 128) and a run of KR_VERIFY_MAX = 16 from position 63 (it crosses the page edge at 64; the interface
    takes no longer run).  The next step still equals the single-sequence reference"""
    st, _, d, prompts, firsts, refs = _get(hd, nh, fp8)
    pt = 32
    i700, i127, i63 = LENS.index(700), LENS.index(127), LENS.index(63)
    st.create_slots(4, SLOT_SEQ, page_tokens=pt, n_pages=_pages(1151, pt) + _pages(132, pt) + _pages(79, pt) + 1)
    _fill_slots(st, d, [prompts[i700]], [[3]])
    dirty = st.slot_page_ids(3)[0][:_pages(700, pt)]
    st.trim_slot(3, 0)                                                      # 22 pages of sequence rows go back to the pool
    _fill_slots(st, d, [prompts[LONG], prompts[i127], prompts[i63]], [[0], [1], [2]])
    assert set(dirty) <= set(st.slot_page_ids(0)[0])                        # ... and the long row holds them now
    st.set_option(OPT, 1)
    rng = np.random.default_rng(5)
    st.verify_multi([1, 2], [[firsts[i127]] + _toks(rng, d, 4), [firsts[i63]] + _toks(rng, d, 15)], [127, 63])
    st.commit_multi([0, 0])
    assert [st.slot_pages()["per_slot"][s] for s in (1, 2)] == [_pages(132, pt), _pages(79, pt)]      # the drafted positions stay mapped, holding rejected rows
    rows = [LONG, i127, i63]
    ids, lg = st.step_multi([0, 1, 2], [firsts[i] for i in rows], [LENS[i] for i in rows], logits=True)
    for r, i in enumerate(rows):
        assert np.array_equal(lg[r].view(U), refs[i][0][0][0]) and ids[r] == refs[i][0][0][1], LENS[i]


# ---- 3: every entry point, against flat slots under "multi_attn_fast" ---------------------------------------------------------------------------------------
SAMPLER = dict(temperature=[0.8, 1.0], top_k=[20, 0], top_p=[0.9, 1.0], presence_penalty=[0.0, 0.5])


def _entry_points(st, d, paged, prompts, firsts, refs, runs, page_tokens=32):
    """one call sequence over every batched entry point, on paged slots under the new option or on flat slots under "multi_attn_fast" -> all it produced"""
    pt = page_tokens
    P = prompts[LONG]
    A, B, C, D = 2, 0, 3, 1                                                 # 1150 positions | 700 | the first 100 of the long prompt | its first 1000
    st.set_option(OPT, 0); st.set_option("multi_attn_fast", 0)
    st.create_slots(4, SLOT_SEQ, **(dict(page_tokens=pt, n_pages=_pages(1200, pt) + _pages(760, pt) + _pages(240, pt) + _pages(1200, pt)) if paged else {}))
    _fill_slots(st, d, [P, prompts[LENS.index(700)], P[:100], P[:1000]], [[A], [B], [C], [D]])
    st.set_option(OPT if paged else "multi_attn_fast", 1)
    out = []
    state = lambda s, n: _slot_state(Gqa, st, d, s, n)
    # runs of 70 tokens from position 100 (over the chunk edge at 128 and into three more pages), of one token, and of 130 tokens
    ids, lg = st.extend_multi([C, B, D], [P[100:170], [firsts[LENS.index(700)]], P[1000:1130]], [100, 700, 1000], logits=True)
    out.append(("extend", list(ids), _bits(lg)))
    pos = {A: 1150, B: 701, C: 170, D: 1130}
    # verify + commit: kept 0, 1 and all
    vr = [runs[0], runs[1], runs[2]]
    ids, nm = st.verify_multi([A, B, C], vr, [pos[A], pos[B], pos[C]])
    keep = [0, 1, nm[2] + 1]
    st.commit_multi(keep)
    out.append(("verify", [g[:m + 1] for g, m in zip(ids, nm)], list(nm)))
    for s, k in zip((A, B, C), keep):
        pos[s] += k
    st.set_slot_sampler(A, runs[0][0], 0.8, 20, 0.9, 0.0, 7); st.set_slot_sampler(D, runs[3][0], 1.0, 0, 1.0, 0.5, 9)
    ids, nm = st.verify_multi_sample([A, D], [runs[0], runs[3]], [pos[A], pos[D]])
    keep = [nm[0] + 1, 1]
    st.commit_multi(keep)
    out.append(("verify_sample", [g[:m + 1] for g, m in zip(ids, nm)], list(nm), [st.slot_sampler_state(s) for s in (A, D)]))
    pos[A] += keep[0]; pos[D] += keep[1]
    # the four generation loops: greedy, greedy with lookup, sampled with two seeds, sampled with lookup
    T = st.generate_multi([A, C], [runs[0][0], runs[2][0]], [pos[A], pos[C]], 5)
    out.append(("generate", T)); pos[A] += len(T[0]); pos[C] += len(T[1])
    T = st.generate_multi_lookup([B, D], [runs[1][0], runs[3][0]], [pos[B], pos[D]], 6, [P[:200], P[:200]], 4, 2)
    out.append(("lookup", T, dict(st.last_multi_lookup_stats))); pos[B] += len(T[0]); pos[D] += len(T[1])
    for seeds in ([11, 12], [0x9E3779B9, 77]):
        T = st.generate_multi([A, B], [runs[0][1], runs[1][1]], [pos[A], pos[B]], 4, rng_seeds=seeds, **SAMPLER)
        out.append(("sample", T, [st.slot_sampler_state(s) for s in (A, B)])); pos[A] += len(T[0]); pos[B] += len(T[1])
    T = st.generate_multi_lookup_sample([C, D], [runs[2][1], runs[3][1]], [pos[C], pos[D]], 5, [P[:200], P[:200]], 4, 2, rng_seeds=[5, 6], **SAMPLER)
    out.append(("lookup_sample", T, dict(st.last_multi_lookup_stats), [st.slot_sampler_state(s) for s in (C, D)])); pos[C] += len(T[0]); pos[D] += len(T[1])
    st.set_option(OPT, 0); st.set_option("multi_attn_fast", 0)
    return out, [state(s, pos[s]) for s in (A, B, C, D)]


def _equal(a, b, where=""):
    if isinstance(a, np.ndarray):
        assert isinstance(b, np.ndarray) and np.array_equal(a, b), where
    elif isinstance(a, (list, tuple)):
        assert len(a) == len(b), where
        for j, (x, y) in enumerate(zip(a, b)):
            _equal(x, y, f"{where}[{j}]")
    else:
        assert a == b, (where, a, b)


@pytest.mark.parametrize("hd,nh,fp8", MODELS)
def test_every_entry_point_equals_the_flat_run(hd, nh, fp8):
    st, _, d, prompts, firsts, refs = _get(hd, nh, fp8)
    rng = np.random.default_rng(6)
    i700 = LENS.index(700)
    # a run = [token, drafts ...]: the long row's own greedy continuation and then a wrong token, so that some drafts match; random drafts elsewhere
    runs = [[firsts[LONG], refs[LONG][0][0][1], refs[LONG][0][1][1], (refs[LONG][0][2][1] + 1) % d["V"]], _toks(rng, d, 4), _toks(rng, d, 6), _toks(rng, d, 3)]
    got, states = _entry_points(st, d, True, prompts, firsts, refs, runs)
    flat, flat_states = _entry_points(st, d, False, prompts, firsts, refs, runs)
    assert [g[0] for g in got] == [f[0] for f in flat]
    for g, f in zip(got, flat):
        _equal(g[1:], f[1:], g[0])
    assert got[1][2][0] == 2 and got[1][1][0] == [refs[LONG][0][k][1] for k in range(3)]      # the verify of the long row against the single-sequence fast reference
    for a, b in zip(states, flat_states):
        _same(a, b)


# ---- 4: forked slots ----------------------------------------------------------------------------------------------------------------------------------------
def _fork_run(st, d, paged, pt, prompts, firsts, toks, new):
    SRC, DSTS, FORK, REWIND = 3, [0, 2], 1100, 1000
    st.set_option(OPT, 0); st.set_option("multi_attn_fast", 0)
    st.create_slots(4, SLOT_SEQ, **(dict(page_tokens=pt, n_pages=_pages(1151, pt) + 2 + _pages(1102, pt) - FORK // pt + 2) if paged else {}))
    _fill_slots(st, d, [prompts[LONG]], [[SRC]])
    st.fork_slot(SRC, DSTS, FORK)
    full = FORK // pt
    if paged:
        tables = [st.slot_page_ids(s) for s in [SRC] + DSTS]
        for ids, refc in tables:
            assert ids[:full] == tables[0][0][:full] and refc[:full] == [3] * full      # whole pages shared by the three slots
        assert len({ids[full] for ids, _ in tables}) == 3 and all(refc[full] == 1 for _, refc in tables)      # a private boundary page each
    st.set_option(OPT if paged else "multi_attn_fast", 1)
    out = []
    ids, lg = st.step_multi(DSTS, toks[:2], [FORK, FORK], logits=True)     # each destination with its own first token
    out.append((list(ids), _bits(lg)))
    ids, lg = st.extend_multi([DSTS[0]], [new], [REWIND], logits=True)      # a write below the fork point: copy-on-write of the pages it lands in
    out.append((list(ids), _bits(lg)))
    if paged:
        ids_d, refc = st.slot_page_ids(DSTS[0])
        hit = range(REWIND // pt, _pages(REWIND + len(new), pt))
        assert all(refc[j] == 1 and ids_d[j] != tables[0][0][j] for j in hit) and all(st.slot_page_ids(SRC)[1][j] == 2 for j in hit)
    ids, lg = st.step_multi([SRC] + DSTS, [firsts[LONG], toks[2], toks[3]], [1150, REWIND + len(new), FORK + 1], logits=True)
    out.append((list(ids), _bits(lg)))
    st.set_option(OPT, 0); st.set_option("multi_attn_fast", 0)
    return out, [_slot_state(Gqa, st, d, s, n) for s, n in ((SRC, 1151), (DSTS[0], REWIND + len(new) + 1), (DSTS[1], FORK + 2))]


@pytest.mark.parametrize("page_tokens", [32, 64])
def test_forked_slots(page_tokens):
    """the 1150-position slot forked at 1100 to two destinations: whole pages shared, a private boundary page each; a step of each destination with its own
    token, a rewind of one by extend_multi from position 1000 (copy-on-write), a step of all three.  Equal to flat forked slots under "multi_attn_fast"; the
    source's step also equals the single-sequence fast reference"""
    st, _, d, prompts, firsts, refs = _get(256, 16, False)
    rng = np.random.default_rng(8)
    toks, new = _toks(rng, d, 4), _toks(rng, d, 20)
    got, states = _fork_run(st, d, True, page_tokens, prompts, firsts, toks, new)
    flat, flat_states = _fork_run(st, d, False, page_tokens, prompts, firsts, toks, new)
    for (ids, lg), (fids, flg) in zip(got, flat):
        assert ids == fids and np.array_equal(lg, flg)
    for a, b in zip(states, flat_states):
        _same(a, b)
    assert np.array_equal(got[2][1][0], refs[LONG][0][0][0]) and got[2][0][0] == refs[LONG][0][0][1]


# ---- 5: batch composition -----------------------------------------------------------------------------------------------------------------------------------
def test_batch_composition():
    """the 1150-position row alone, as row 0 of a 33-row batch of the other lengths, as its last row, and permuted: the same bits.  The grid's chunk count
    follows the longest row; the workgroups of shorter rows past their end leave"""
    st, _, d, prompts, firsts, refs = _get(256, 16, False)
    pt = 64
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
    st.create_slots(4 + 3 * n_other, SLOT_SEQ, page_tokens=pt, n_pages=sum(_pages(LENS[q] + 1, pt) * len(s) for q, s in enumerate(per_seq)))
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
    assert st.slot_pages()["free"] == 0


# ---- 6: short slots -----------------------------------------------------------------------------------------------------------------------------------------
def test_short_paged_slots_keep_the_exact_step():
    """paged slots of max_seq 1000 <= gqa_split_min: the exact paged kernel runs, the option-off bits (the capacity rule of the flat option)"""
    st, _, d, prompts, firsts, refs = _get(256, 16, False)
    short = [i for i, n in enumerate(LENS) if n <= 700]
    n, pt = len(short), 32
    st.create_slots(2 * n, 1000, page_tokens=pt, n_pages=2 * sum(_pages(LENS[i] + N_STEPS, pt) for i in short))
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
        _same(_slot_state(Gqa, st, d, j, LENS[i] + N_STEPS), _slot_state(Gqa, st, d, n + j, LENS[i] + N_STEPS))


# ---- 7: the stated tolerance against the exact paged step ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hd,nh,fp8", [(256, 16, False), (128, 8, True)])
def test_within_stated_tolerance_of_the_exact_paged_step(hd, nh, fp8):
    """STATED TOLERANCE (02-numerics.md section 2b): max |on - off| <= 1e-3 max |off| on every row's logits, same greedy ids; rows of 700 positions or more
    differ from the exact bits somewhere (no silent fall-back to the exact paged kernel).  Largest ratio observed on an MI355X: 3.65e-4 (head_dim 256 FP16), 3.70e-4 (head_dim 128 E4M3)"""
    st, _, d, prompts, firsts, refs = _get(hd, nh, fp8)
    n, pt = len(LENS), 64
    st.create_slots(2 * n, SLOT_SEQ, page_tokens=pt, n_pages=2 * sum(_pages(m + N_STEPS, pt) for m in LENS))
    _fill_slots(st, d, prompts, [[i, n + i] for i in range(n)])
    toks, pos, exact = list(firsts), [len(p) for p in prompts], []
    for k in range(N_STEPS):
        ids, lg = st.step_multi(list(range(n)), toks, pos, logits=True)
        exact.append((toks, ids, lg)); toks = ids; pos = [p + 1 for p in pos]
    st.set_option(OPT, 1)
    pos, worst, differs = [len(p) for p in prompts], 0.0, False
    for k, (fed, ids_e, lg_e) in enumerate(exact):
        ids, lg = st.step_multi(list(range(n, 2 * n)), fed, pos, logits=True)
        for i in range(n):
            worst = max(worst, float(np.abs(lg[i] - lg_e[i]).max() / np.abs(lg_e[i]).max()))
            if LENS[i] >= 700:
                differs |= not np.array_equal(lg[i].view(U), lg_e[i].view(U))
        print(f"paged hd {hd} fp8 {fp8} step {k}: largest max|on - off| / max|off| so far {worst:.3e} (bound 1e-3)")
        for i in range(n):
            assert float(np.abs(lg[i] - lg_e[i]).max()) <= 1e-3 * float(np.abs(lg_e[i]).max()), (k, LENS[i])
        assert ids == ids_e, k
        pos = [p + 1 for p in pos]
    assert differs, "no long row differs from the exact step in its bits: the flash-decode did not run"


# ---- 8: long rows -------------------------------------------------------------------------------------------------------------------------------------------
LONG_LENS = (700, 2500, 8300)


@functools.lru_cache(maxsize=None)
def _long_model(hd, nh, fp8):
    """a GQA-only store, three injected random states and their single-sequence fast references (two steps): built once, shared by both page sizes"""
    st, keep, d = Gqa.build(fp8, seed=3, hd=hd, nh=nh, kv_max=8448, kinds=["gqa", "gqa"])
    _stores.append(st)
    rng = np.random.default_rng(78)
    states = SC._states(Gqa, d, rng, 3)
    firsts = _toks(rng, d, 3)
    refs = []
    for s, f, n in zip(states, firsts, LONG_LENS):
        SC._inject(Gqa, st, d, s)
        st.set_attention_mode(True)
        try:
            out, tok = [], f
            for k in range(2):
                st.decode_step(tok, n + k)
                out.append((_bits(st.read_logits()), st.last_token())); tok = out[-1][1]
            refs.append((out, _snap(st, d, n + 2)))
        finally:
            st.set_attention_mode(False)
    return st, keep, d, states, firsts, refs


@pytest.mark.parametrize("page_tokens", [32, 256])
@pytest.mark.parametrize("hd,nh,fp8", [(256, 16, False), (64, 4, True)])
def test_long_rows(hd, nh, fp8, page_tokens):
    """rows of 700, 2500 and 8300 positions (65 chunks, 260 table entries at page_tokens 32) from injected states, in one step; the longest row's pages are
    not contiguous.  Reference: decode_step under set_attention_mode(True) from the same injected state"""
    st, keep, d, states, firsts, refs = _long_model(hd, nh, fp8)
    pt = page_tokens
    slots, spare = [2, 0, 3], 1
    st.create_slots(4, max(LONG_LENS) + 40, page_tokens=pt, n_pages=sum(_pages(n + 2, pt) for n in LONG_LENS))
    SC._inject(Gqa, st, d, states[0]); st.save_slot(slots[0], LONG_LENS[0])
    st.save_slot(spare, 100)
    SC._inject(Gqa, st, d, states[1]); st.save_slot(slots[1], LONG_LENS[1])
    st.trim_slot(spare, 0)
    SC._inject(Gqa, st, d, states[2]); st.save_slot(slots[2], LONG_LENS[2])
    used = st.slot_page_ids(slots[2])[0][:_pages(LONG_LENS[2], pt)]
    assert min(used) >= 0 and len(set(np.diff(used).tolist())) > 1
    st.set_option(OPT, 1)
    toks, pos = list(firsts), list(LONG_LENS)
    for k in range(2):
        got, lg = st.step_multi(slots, toks, pos, logits=True)
        for i, (ref, _) in enumerate(refs):
            assert np.array_equal(lg[i].view(U), ref[k][0]), ("logits", k, i)
            assert got[i] == ref[k][1], ("id", k, i)
        toks = got; pos = [p + 1 for p in pos]
    st.set_option(OPT, 0)
    for i, (_, snap) in enumerate(refs):
        _same(_slot_state(Gqa, st, d, slots[i], pos[i]), snap)


# ---- 9: chunks of 256 positions -----------------------------------------------------------------------------------------------------------------------------
def test_chunk_of_256_positions():
    """a store and slots of more than 131 072 positions: a chunk is 256 positions and spans 8 table entries at page_tokens 32.  Rows of 300 and 600
    positions against the store's own fast step"""
    kv_max = 131072 + 128
    st, keep, d = Gqa.build(True, seed=3, hd=64, nh=4, kv_max=kv_max)
    _stores.append(st)
    rng = np.random.default_rng(9)
    prompts, firsts = [_toks(rng, d, 300), _toks(rng, d, 600)], _toks(rng, d, 2)
    refs = []
    for p, f in zip(prompts, firsts):
        refs.append(_fast_reference(st, d, p, f, 2))
    st.create_slots(3, kv_max, page_tokens=32, n_pages=36)
    _fill_slots(st, d, prompts[:1], [[2]])
    st.save_slot(1, 40)
    _fill_slots(st, d, prompts[1:], [[0]])
    st.set_option(OPT, 1)
    toks, pos = list(firsts), [300, 600]
    for k in range(2):
        ids, lg = st.step_multi([2, 0], toks, pos, logits=True)
        for i, (ref, _) in enumerate(refs):
            assert np.array_equal(lg[i].view(U), ref[k][0]) and ids[i] == ref[k][1], (k, i)
        toks = ids; pos = [p + 1 for p in pos]
    st.set_option(OPT, 0)
    for i, s in enumerate((2, 0)):
        _same(_slot_state(Gqa, st, d, s, pos[i]), refs[i][1])


# ---- 10: refusals and unchanged behaviour -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("paged", [True, False])
def test_mla_stores_are_refused_under_the_option(paged):
    """a store with MLA layers: every batched call is refused with KR_ERR_STATE naming the option that is set, and changes nothing"""
    import tests.test_multi_mla_gpu as MM
    st, eng, keep, d = MM._build(kv_max=48)
    _stores.append(st)
    rng = np.random.default_rng(3)
    prompt = MM._prompt(rng, d, 20)
    ref, _ = MM._reference(st, d, prompt, 2, 1)
    st.create_slots(2, 40, **(dict(page_tokens=32, n_pages=4) if paged else {}))
    MM._fill_slots(st, d, [prompt], [[1]])
    want_slot = MM._snap(st, d, 20)
    before = st.slot_pages()
    st.decode_step(5, 20)
    want_lg, want_tok = _bits(st.read_logits()), st.last_token()
    for both in (0, 1):
        st.set_option(OPT, 1); st.set_option("multi_attn_fast", both)
        for call in (lambda: st.step_multi([1], [2], [20]), lambda: st.generate_multi([1], [2], [20], 2), lambda: st.step_multi_sample([1], [2], [20]),
                     lambda: st.extend_multi([0], [[1, 2]], [0]), lambda: st.verify_multi([1], [[2, 3]], [20]), lambda: st.generate_multi_lookup([1], [2], [20], 2),
                     lambda: st.generate_multi([1], [2], [20], 2, temperature=0.6, rng_seeds=3)):
            _state_error(call, OPT)
            assert np.array_equal(st.read_logits().view(U), want_lg) and st.last_token() == want_tok
            assert st.slot_pages() == before
    st.set_option(OPT, 0); st.set_option("multi_attn_fast", 0)
    st.reset_decode_state(d["kv_max"]); st.load_slot(1, 20)
    MM._same(MM._snap(st, d, 20), want_slot)
    ids, lg = st.step_multi([1], [2], [20], logits=True)
    assert np.array_equal(lg[0].view(U), ref[0][0]) and ids[0] == ref[0][1]


def test_options_across_flat_and_paged_slots():
    """"multi_attn_fast" alone on paged slots stays refused, naming both; with both options set the new one governs; on flat slots the new option alone gives
    the bits of "multi_attn_fast"; a call the pool cannot supply -- a step of two rows and an extend of two runs that each need one page where one is free --
    is refused whole with the option on, pages and slot state unchanged"""
    st, _, d, prompts, firsts, refs = _get(64, 4, False)
    i = LENS.index(700)
    pt = 32
    st.create_slots(2, SLOT_SEQ, page_tokens=pt, n_pages=2 * _pages(700, pt) + 1)      # 700 positions = 22 pages that end at position 703: position 704 needs a 23rd
    _fill_slots(st, d, [prompts[i]], [[0, 1]])
    want = _slot_state(Gqa, st, d, 0, 700)
    before = st.slot_pages()
    assert before["free"] == 1
    st.set_option("multi_attn_fast", 1)
    for call in (lambda: st.step_multi([1], [2], [700]), lambda: st.extend_multi([0], [[1, 2]], [700]), lambda: st.generate_multi([1], [2], [700], 4),
                 lambda: st.verify_multi([1], [[2, 3]], [700]), lambda: st.generate_multi_lookup([1], [2], [700], 4)):
        _state_error(call, "multi_attn_fast", "paged")
    assert st.slot_pages() == before
    st.set_option(OPT, 1)                                                   # both set: the new one governs
    # each slot needs its 23rd page for positions [700, 705): two pages, one is free -- refused whole
    _state_error(lambda: st.extend_multi([0, 1], [_toks(np.random.default_rng(1), d, 5)] * 2, [700, 700]), "row 1", "slot 1")
    assert st.slot_pages() == before
    _state_error(lambda: st.step_multi([0, 1], [3, 4], [704, 704]), "row 1", "slot 1")      # the same as a step: both rows at the first position of a 23rd page
    assert st.slot_pages() == before
    for s in (0, 1):
        _same(_slot_state(Gqa, st, d, s, 700), want)
    ids, lg = st.step_multi([0], [firsts[i]], [700], logits=True)
    assert np.array_equal(lg[0].view(U), refs[i][0][0][0]) and ids[0] == refs[i][0][0][1]
    st.set_option("multi_attn_fast", 0)                                     # the new option alone
    ids, lg = st.step_multi([1], [firsts[i]], [700], logits=True)
    assert np.array_equal(lg[0].view(U), refs[i][0][0][0]) and ids[0] == refs[i][0][0][1]
    st.create_slots(2, SLOT_SEQ)                                            # flat slots, the new option alone: the bits of "multi_attn_fast"
    _fill_slots(st, d, [prompts[i]], [[0, 1]])
    ids, lg = st.step_multi([1], [firsts[i]], [700], logits=True)
    assert np.array_equal(lg[0].view(U), refs[i][0][0][0]) and ids[0] == refs[i][0][0][1]
    st.set_option(OPT, 0)
    st.decode_step(firsts[i], 700)                                          # both off: the exact step (the store still holds the prompt's state)
    exact_lg, exact_tok = _bits(st.read_logits()), st.last_token()
    ids, lg = st.step_multi([0], [firsts[i]], [700], logits=True)
    assert np.array_equal(lg[0].view(U), exact_lg) and ids[0] == exact_tok
