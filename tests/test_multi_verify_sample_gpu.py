"""Exact sampled speculation over device slots (kr_decode_verify_multi_sample / kr_decode_commit_multi / kr_decode_generate_multi_lookup_sample,
kr_sample_runs; docs/design/19-multi-verify-sample.md): a sampled verify of [sampled token, draft] runs gives after every token the id
step_multi_sample gives there, and a commit of n_keep tokens leaves each slot AND its sampler (seen bitmap, xorshift64 state) as n_keep
step_multi_sample calls leave them.  The yardsticks are the numpy oracle's sampler, chained per run, and step_multi_sample token by token on a twin
slot; every assertion is on ids, u64 states, bitmaps and u32 bit patterns -- no tolerances."""
import ctypes as C

import numpy as np
import pytest

from krasis_amd._lib import KR_VERIFY_MAX
from tests.test_decode_gpu import build
from tests.test_speculative_gpu import _same, _snap
from tests.test_multi_seq_gpu import LA4
from tests.test_multi_extend_gpu import _slot_state, _toks
from tests.test_multi_sample_gpu import ROW_PARAMS, _gen_params, _oracle_row
from tests.test_multi_verify_gpu import ROWS, SLOTS, _fill, _wrong_at
from tests import test_multi_mla_gpu as mla

pytestmark = pytest.mark.gpu
F = np.float32
U = np.uint32


# ---- kr_sample_runs against the oracle's sampler ----------------------------------------------------------------------------------------------------
def _sample_runs(lg, counts, tokens, params, seen, states, n_keep, force_loop=False):
    from krasis_amd import _lib
    lib = _lib.load_library()
    n, (T, V) = len(counts), lg.shape
    col = lambda j, t: np.ascontiguousarray([p[j] for p in params], t)
    TE, K, P, PEN = col(0, F), col(1, np.int32), col(2, F), col(3, F)
    cn, tk = np.ascontiguousarray(counts, np.int32), np.ascontiguousarray(tokens, np.int32)
    sn, rng, keep = seen.copy(), np.ascontiguousarray(states, np.uint64), np.ascontiguousarray(n_keep, np.int32)
    ids, nm = np.empty(T, np.int32), np.empty(n, np.int32)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    rc = lib.kr_sample_runs(ptr(lg), n, ptr(cn), ptr(tk), V, ptr(TE), ptr(K), ptr(P), ptr(PEN), ptr(sn), ptr(rng), ptr(keep), ptr(ids), ptr(nm), int(force_loop))
    assert rc == 0, lib.kr_last_error()
    offs = np.concatenate([[0], np.cumsum(counts)])
    return [[int(x) for x in ids[offs[i]:offs[i + 1]]] for i in range(n)], [int(x) for x in nm], sn, [int(x) for x in rng], [int(x) for x in keep]


def _marks(params):
    return params[0] > 0 or params[3] != 0.0          # every mode but plain greedy marks its token seen


def _oracle_chain(rows, params, mask, state):
    """kr_decode_generate's loop on the rows of one run: draw, mark, go on.  ids[t], and masks[t] / states[t] = the sampler after t draws"""
    mask = mask.copy()
    ids, masks, states = [], [mask.copy()], [state]
    for lg in rows:
        tok, state = _oracle_row(lg, params, mask[:lg.size], state)
        if _marks(params):
            mask[tok] = True
        ids.append(tok); masks.append(mask.copy()); states.append(state)
    return ids, masks, states


def _bitmap(mask):
    n, bits = mask.shape
    return np.packbits(mask.reshape(n, bits // 32, 32), axis=-1, bitorder="little").reshape(n, bits // 8).view(U)


COUNTS = [1, 2, 5, 16, 3, 9, 1, 7, 4]
WRONG = [None, 1, 3, None, 2, 5, None, None, 1]          # index of the injected wrong draft per run


@pytest.mark.parametrize("V", [151936, 1007])
def test_sample_runs_match_the_oracle(V):
    n, T, W = len(COUNTS), sum(COUNTS), (V + 31) // 32
    rng = np.random.default_rng(V)
    lg = (rng.integers(-200, 200, (T, V)).astype(F) * F(0.125)).astype(F)      # coarse grid: the k-th value is tied across the cut
    for b in range(T):
        lg[b, rng.integers(0, V, 3)] = F(-0.0)                                # signed zeros compare equal
    lg[:, 7] = lg.max() + F(1)
    lg[::2, 7] = lg[::2, 9] = lg.max()                                        # a tie of two maxima in every other row
    params = list(ROW_PARAMS)
    mask = rng.random((n, W * 32)) < 0.02                                     # random seen sets
    mask[:, 7] = rng.random(n) < 0.5
    states = [int(x) for x in rng.integers(1, 2**63, n)]
    offs = np.concatenate([[0], np.cumsum(COUNTS)])
    tokens, want = [], []
    for i, c in enumerate(COUNTS):
        ids, masks, sts = _oracle_chain(lg[offs[i]:offs[i + 1]], params[i], mask[i], states[i])
        run = [int(rng.integers(0, V))] + ids[:c - 1]                         # the drafts: the oracle's own chain ...
        m = c - 1
        if WRONG[i] is not None:                                              # ... with a wrong token at one index
            run[WRONG[i]] = (run[WRONG[i]] + 1) % V
            m = WRONG[i] - 1
        tokens += run; want.append((ids, m, masks, sts))
    # the inputs cover: nothing accepted, a part accepted, everything accepted
    assert any(m == 0 and c > 1 for (_, m, _, _), c in zip(want, COUNTS))
    assert any(0 < m < c - 1 for (_, m, _, _), c in zip(want, COUNTS))
    assert any(m == c - 1 and c > 1 for (_, m, _, _), c in zip(want, COUNTS))
    seen = _bitmap(mask)
    for keep_of in (lambda m: 0, lambda m: 1, lambda m: m + 1):
        keep = [keep_of(m) for _, m, _, _ in want]
        got = _sample_runs(lg, COUNTS, tokens, params, seen, states, keep)
        for i, (ids, m, masks, sts) in enumerate(want):
            assert got[1][i] == m, ("n_match", i, got[1])
            assert got[0][i][:m + 1] == ids[:m + 1], ("ids", i)
            assert got[4][i] == keep[i]
            assert np.array_equal(got[2][i], _bitmap(masks[keep[i]][None])[0]), ("bitmap", i, keep[i])
            assert got[3][i] == sts[keep[i]], ("rng", i, keep[i])
        loop = _sample_runs(lg, COUNTS, tokens, params, seen, states, keep, force_loop=True)
        for i, (ids, m, _, _) in enumerate(want):
            assert loop[0][i][:m + 1] == got[0][i][:m + 1], ("loop ids", i)
        assert loop[1] == got[1] and np.array_equal(loop[2], got[2]) and loop[3:] == got[3:]
    got = _sample_runs(lg, COUNTS, tokens, params, seen, states, [-1] * n)   # negative: everything accepted is kept
    assert got[4] == [m + 1 for _, m, _, _ in want]


@pytest.mark.parametrize("params", [(0.0, 0, 1.0, 1.5), (1.0, 1, 1.0, 1.5)])
@pytest.mark.parametrize("A,B,old", [(37, 101, None), (37, 101, 35)])         # old: an already seen token in A's bitmap word
def test_a_prefix_token_changes_a_later_draw(params, A, B, old):
    """token A beats token B by less than the penalty: once A is a draft before the row, the row draws B"""
    V, x = 200, 150
    W = (V + 31) // 32
    row = np.full(V, -3.0, F); row[A] = 5.0; row[B] = 4.0
    lg = np.stack([row] * 3)
    mask = np.zeros((1, W * 32), bool)
    if old is not None:
        mask[0, old] = True
    seen = _bitmap(mask)
    for force_loop in (False, True):
        ids, nm, sn, st, keep = _sample_runs(lg, [3], [x, A, B], [params], seen, [99], [-1], force_loop)
        assert ids[0][:2] == [A, B] and nm == [2] and ids[0][2] == A, ids     # after A and B: A - 1.5 > B - 1.5
        after = mask.copy(); after[0, [A, B, A]] = True
        assert np.array_equal(sn, _bitmap(after)) and keep == [3]
        ids, nm, sn, st, keep = _sample_runs(lg, [3], [x, A, A], [params], seen, [99], [-1], force_loop)
        assert ids[0][:2] == [A, B] and nm == [1], ids
        after = mask.copy(); after[0, [A, B]] = True
        assert np.array_equal(sn, _bitmap(after)) and keep == [2]
    # a repeated prefix token is penalised once: A - 1.5 still beats B' = 3, A - 3 would not
    row2 = row.copy(); row2[B] = 3.0
    ids, nm, _, _, _ = _sample_runs(np.stack([row2] * 3), [3], [x, A, A], [params], seen, [99], [-1])
    assert ids[0] == [A, A, A] and nm == [2]


# ---- model level: twin slots ------------------------------------------------------------------------------------------------------------------------
def _smp_same(a, b):
    assert a[1] == b[1], "rng state"
    assert np.array_equal(a[0], b[0]), "seen bitmap"


def _strace(st, d, prompt, first, n, test_slot, ref_slot, params, seed, at=(), snap=_snap):
    """the prompt into both slots, the same sampler on both; the reference slot then draws n tokens by step_multi_sample, one at a time.  toks[k] = the
    token step k consumes, smp[k] = the reference's sampler after k steps, snaps[k] (k in `at`) = its slot state after k steps"""
    st.reset_decode_state(d["kv_max"])
    for i, t in enumerate(prompt):
        st.decode_step(t, i)
    p0 = len(prompt)
    for s in (test_slot, ref_slot):
        st.save_slot(s, p0)
        st.set_slot_sampler(s, first, *params, seed)
    tr = dict(p0=p0, toks=[first], smp=[st.slot_sampler_state(ref_slot)], snaps={}, ref=ref_slot)
    for k in range(n + 1):
        if k in at:
            tr["snaps"][k] = _slot_state(st, d, ref_slot, p0 + k, snap)
        if k < n:
            tr["toks"].append(st.step_multi_sample([ref_slot], [tr["toks"][k]], [p0 + k])[0])
            tr["smp"].append(st.slot_sampler_state(ref_slot))
    return tr


def _check(st, d, slot, tr, k, snap=_snap, same=_same):
    same(_slot_state(st, d, slot, tr["p0"] + k, snap), tr["snaps"][k])
    _smp_same(st.slot_sampler_state(slot), tr["smp"][k])


def _all_right(st, d, snap=_snap, same=_same):
    rng = np.random.default_rng(5)
    params, seeds = _gen_params(len(ROWS))
    trs = [_strace(st, d, _toks(rng, d, p), _toks(rng, d, 1)[0], c + 1, s, 7 + i, params[i], seeds[i], (c,), snap)
           for i, ((p, c), s) in enumerate(zip(ROWS, SLOTS))]
    runs = [tr["toks"][:c] for tr, (_, c) in zip(trs, ROWS)]
    ids, nm = st.verify_multi_sample(SLOTS, runs, [tr["p0"] for tr in trs])
    for i, (tr, (_, c)) in enumerate(zip(trs, ROWS)):
        assert ids[i] == tr["toks"][1:c + 1], ("ids", i)
        assert nm[i] == c - 1, ("n_match", i)
    st.commit_multi([c for _, c in ROWS])
    for tr, (_, c), s in zip(trs, ROWS, SLOTS):
        _check(st, d, s, tr, c, snap, same)
    nxt = st.step_multi_sample(SLOTS, [g[-1] for g in ids], [tr["p0"] + c for tr, (_, c) in zip(trs, ROWS)])
    assert nxt == [tr["toks"][c + 1] for tr, (_, c) in zip(trs, ROWS)]        # the slots and their samplers continue as the references do


@pytest.mark.parametrize("loop", [0, 1])
@pytest.mark.parametrize("cfg", [dict(), LA4, dict(fp8=True), dict(mla=True)], ids=["default", "la4", "fp8", "mla"])
def test_all_drafts_right(cfg, loop):
    if cfg.get("mla"):
        st, eng, keep, d = mla._build(False, kv_max=64, **mla.CFGS[1])
        snap, same = mla._snap, mla._same
    else:
        st, eng, orc, keep, d = build(kv_max=64, **{k: v for k, v in cfg.items() if k != "fp8"})
        snap, same = _snap, _same
        if cfg.get("fp8"):
            st.set_kv_dtype(True); d["fp8"] = True
    st.set_option("multi_sample_loop", loop)
    st.create_slots(12, 60)
    _all_right(st, d, snap, same)


@pytest.mark.parametrize("loop", [0, 1])
def test_partial_acceptance_mixed_in_one_call(loop):
    """the first wrong draft at another index per row; one row is accepted whole and keeps nothing"""
    st, eng, orc, keep, d = build(kv_max=64)
    st.set_option("multi_sample_loop", loop)
    st.create_slots(12, 60)
    rng = np.random.default_rng(7)
    js, slots, pre, c = [1, 2, 3, 5, 7], [4, 1, 5, 0, 3, 2], [3, 0, 11, 6, 20, 2], 9
    params, seeds = _gen_params(6)
    trs = [_strace(st, d, _toks(rng, d, p), _toks(rng, d, 1)[0], c, s, 6 + i, params[i], seeds[i], (j,))
           for i, (p, s, j) in enumerate(zip(pre, slots, js + [0]))]
    runs = [_wrong_at(tr, c, j, d["V"]) for tr, j in zip(trs, js)] + [trs[5]["toks"][:c]]
    pos = [tr["p0"] for tr in trs]
    ids, nm = st.verify_multi_sample(slots, runs, pos)
    for i, j in enumerate(js):
        assert nm[i] == j - 1, (i, nm)
        assert ids[i][:j] == trs[i]["toks"][1:j + 1], i
    assert nm[5] == c - 1 and ids[5] == trs[5]["toks"][1:c + 1]
    st.commit_multi(js + [0])
    for tr, j, s in zip(trs, js + [0], slots):
        _check(st, d, s, tr, j)                                               # row 5, n_keep = 0: slot and sampler as before the verify
    nxt = st.step_multi_sample(slots[:5], [tr["toks"][j] for tr, j in zip(trs, js)], [p + j for p, j in zip(pos, js)])
    assert nxt == [tr["toks"][j + 1] for tr, j in zip(trs, js)]


@pytest.mark.parametrize("loop", [0, 1])
def test_truncated_commit(loop):
    st, eng, orc, keep, d = build(kv_max=64, seed=2)
    st.set_option("multi_sample_loop", loop)
    st.create_slots(8, 60)
    rng = np.random.default_rng(9)
    keeps, slots, c = [1, 3, 6], [5, 2, 0], 9
    params, seeds = _gen_params(5)
    trs = [_strace(st, d, _toks(rng, d, p), _toks(rng, d, 1)[0], c, s, ref, params[i + 2], seeds[i + 2], (k,))
           for i, (p, s, ref, k) in enumerate(zip([4, 0, 9], slots, [7, 6, 4], keeps))]
    ids, nm = st.verify_multi_sample(slots, [tr["toks"][:c] for tr in trs], [tr["p0"] for tr in trs])
    assert nm == [c - 1] * 3
    st.commit_multi(keeps)                                                    # fewer than the verify accepted
    for tr, k, s in zip(trs, keeps, slots):
        _check(st, d, s, tr, k)
    nxt = st.step_multi_sample(slots, [tr["toks"][k] for tr, k in zip(trs, keeps)], [tr["p0"] + k for tr, k in zip(trs, keeps)])
    assert nxt == [tr["toks"][k + 1] for tr, k in zip(trs, keeps)]


def test_the_verify_writes_nothing():
    """a sampled verify dropped by commit_multi([0, ...]) leaves every slot and sampler as it was, and neither call touches the store's own sequence,
    logits or sampler"""
    st, eng, orc, keep, d = build(kv_max=48)
    rng = np.random.default_rng(41)
    prompt, others = _toks(rng, d, 6), [_toks(rng, d, 4), _toks(rng, d, 11), _toks(rng, d, 2)]
    tok0, pos = 17, len(prompt)
    smp = dict(temperature=0.6, top_k=50, top_p=0.95, presence_penalty=0.5)
    st.create_slots(3, 48)
    _fill(st, d, others, [[0], [1], [2]])
    st.set_slot_sampler(0, 3, 0.6, 50, 0.95, 0.5, 99)
    st.set_slot_sampler(1, 4, 0.0, 0, 1.0, 1.5, 98)
    st.set_slot_sampler(2, 5, 1.3, 0, 0.8, 0.0, 97)
    plen = [len(o) for o in others]
    state = lambda: [(_slot_state(st, d, s, p), st.slot_sampler_state(s)) for s, p in zip(range(3), plen)]
    before = state()

    def run(between):
        st.reset_decode_state(d["kv_max"])
        st.prefill(prompt, 0)
        st.decode_step(tok0, pos)
        a = st.sample(**smp, rng_seed=0xC0FFEE, reset_seen=True)
        between()
        lg0, last = st.read_logits().view(U).copy(), st.last_token()
        st.decode_step(a, pos + 1)
        return a, lg0, last, st.read_logits().view(U).copy(), st.sample(**smp, rng_seed=0)   # continues the store's RNG state and seen set

    ref = run(lambda: None)

    def dropped_verify():
        ids, nm = st.verify_multi_sample([2, 0, 1], [[5, 1, 2, 3], [3, 9], [4, 8, 8, 8, 8, 8]], plen[2:] + plen[:2])
        st.commit_multi([0, 0, 0])

    got = run(dropped_verify)
    assert got[0] == ref[0] and got[2] == ref[2] and got[4] == ref[4]
    assert np.array_equal(got[1], ref[1]) and np.array_equal(got[3], ref[3])
    for (sa, ma), (sb, mb) in zip(state(), before):
        _same(sa, sb); _smp_same(ma, mb)


def test_independence_of_rows():
    """six rows permuted in one call: every row as in a call of that row alone"""
    st, eng, orc, keep, d = build(kv_max=64)
    st.create_slots(12, 60)
    rng = np.random.default_rng(13)
    rows = [(0, 1, None), (0, 9, 4), (7, 5, None), (23, 1, None), (2, 8, 2), (4, 16, 11)]      # (prompt, run length, index of a wrong draft)
    slots = [3, 0, 5, 2, 4, 1]
    params, seeds = _gen_params(6)
    runs, pos, alone = [], [], []
    for i, ((p, c, j), s) in enumerate(zip(rows, slots)):
        tr = _strace(st, d, _toks(rng, d, p), _toks(rng, d, 1)[0], c, s, 6 + i, params[i], seeds[i])
        run = tr["toks"][:c] if j is None else _wrong_at(tr, c, j, d["V"])
        st.set_slot_sampler(6 + i, tr["toks"][0], *params[i], seeds[i])      # the twin again, from the start: load the prompt state back into it
        st.reset_decode_state(d["kv_max"]); st.load_slot(s, p); st.save_slot(6 + i, p)
        g, m = st.verify_multi_sample([6 + i], [run], [p])
        st.commit_multi([m[0] + 1])
        alone.append((g[0][:m[0] + 1], m[0], _slot_state(st, d, 6 + i, p + m[0] + 1), st.slot_sampler_state(6 + i)))
        runs.append(run); pos.append(p)
    assert [m for _, m, _, _ in alone] == [0, 3, 4, 0, 1, 10]
    order = [5, 2, 0, 4, 1, 3]
    pick = lambda xs: [xs[i] for i in order]
    ids, nm = st.verify_multi_sample(pick(slots), pick(runs), pick(pos))
    st.commit_multi([m + 1 for m in nm])
    for r, i in enumerate(order):
        assert nm[r] == alone[i][1] and ids[r][:nm[r] + 1] == alone[i][0], ("alone", i)
        _same(_slot_state(st, d, slots[i], pos[i] + nm[r] + 1), alone[i][2])
        _smp_same(st.slot_sampler_state(slots[i]), alone[i][3])


def _lookup_equals_generate(st, d, n_rows, max_draft, cases, check_stats):
    """twin slots A / B: generate_multi_lookup_sample on A against the sampled generate_multi on B -- tokens, slot states, sampler states"""
    rng = np.random.default_rng(23)
    n_tok = 12
    prompts = [_toks(rng, d, p) for p in (5, 0, 9, 3, 60 - n_tok)[-n_rows:]]  # the last row ends at the slot boundary
    firsts, pos = _toks(rng, d, n_rows), [len(p) for p in prompts]
    A, B = [6, 1, 4, 3, 8][:n_rows], [0, 7, 2, 5, 9][:n_rows]
    params, seeds = _gen_params(n_rows)                                       # sampled, plain greedy, penalised sampled, penalised greedy(, top_k 0)
    smp = dict(temperature=[p[0] for p in params], top_k=[p[1] for p in params], top_p=[p[2] for p in params],
               presence_penalty=[p[3] for p in params], rng_seeds=seeds)
    for repeat, stop in cases:
        _fill(st, d, prompts, [[a, b] for a, b in zip(A, B)])
        want = st.generate_multi(B, firsts, pos, n_tok, **smp)
        stops = ()
        if stop:      # a stop id that row 0 first emits at index k >= 2: inside the draft its first pass accepts (max_draft 1: in a later pass)
            k = next(k for k in range(2, n_tok) if want[0].index(want[0][k]) == k)
            stops = (want[0][k],)
            _fill(st, d, prompts, [[b] for b in B])
            want = st.generate_multi(B, firsts, pos, n_tok, stop_ids=stops, **smp)
            assert len(want[0]) == k + 1
        # contexts that hold the row's own sampled stream (every draft right), or contexts that do not
        ctx = [[f] + w for f, w in zip(firsts, want)] if repeat else [_toks(rng, d, 20) for _ in range(n_rows)]
        got = st.generate_multi_lookup_sample(A, firsts, pos, n_tok, contexts=ctx, max_draft=max_draft, stop_ids=stops, **smp)
        assert got == want
        for a, b, p, w in zip(A, B, pos, want):
            _same(_slot_state(st, d, a, p + len(w)), _slot_state(st, d, b, p + len(w)))
            _smp_same(st.slot_sampler_state(a), st.slot_sampler_state(b))
        if repeat:
            check_stats(st.last_multi_lookup_stats, n_tok)


@pytest.mark.parametrize("max_draft", [1, 4, 15])
def test_generate_multi_lookup_sample_equals_generate_multi(max_draft):
    st, eng, orc, keep, d = build(kv_max=64, seed=1)
    st.create_slots(10, 60)

    def speculated(stats, n_tok):
        assert stats["passes"] < n_tok and all(a > 0 for a in stats["accepted"]), stats

    _lookup_equals_generate(st, d, 4, max_draft, ((True, False), (False, False), (True, True)), speculated)


def test_generate_multi_lookup_sample_with_a_row_on_the_per_row_path():
    """a vocabulary above KR_MS_SEL_CAP: the top_k 0 row takes the per-row path (KR_MS_LOOP), does not draft and rides along with count 1 -- so the
    call takes a pass per token -- beside sampled, plain greedy, penalised sampled and penalised greedy rows that speculate"""
    st, eng, orc, keep, d = build(kv_max=64, seed=1, dims=(256, 4608, 16, 4, 128, 128))
    st.create_slots(10, 60)

    def rode_along(stats, n_tok):
        assert all(a > 0 for a in stats["accepted"][:4]) and stats["accepted"][4] == 0 and stats["passes"] == n_tok, stats

    _lookup_equals_generate(st, d, 5, 4, ((True, False), (True, True)), rode_along)
    st.set_option("multi_sample_loop", 1)                                     # every sampled row on the per-row path: no row but the greedy ones drafts
    _lookup_equals_generate(st, d, 5, 4, ((True, False),), lambda stats, n_tok: None)


def test_greedy_is_untouched():
    st, eng, orc, keep, d = build(kv_max=64)
    st.create_slots(8, 60)
    rng = np.random.default_rng(5)
    prompts = [_toks(rng, d, p) for p, _ in ROWS]
    runs = [_toks(rng, d, c) for _, c in ROWS]
    pos = [len(p) for p in prompts]
    _fill(st, d, prompts, [[s] for s in SLOTS])
    want = st.verify_multi(SLOTS, runs, pos)
    st.commit_multi([0] * 5)
    got = st.verify_multi_sample(SLOTS, runs, pos)                            # no slot has a sampler: every row is plain greedy
    st.commit_multi([0] * 5)
    assert got == want
    zero = st.slot_sampler_state(SLOTS[0])
    assert not zero[0].any() and zero[1] == 0
    params, seeds = _gen_params(5)
    for s, r, p, seed in zip(SLOTS, runs, params, seeds):
        st.set_slot_sampler(s, r[0], *p, seed)
    assert st.verify_multi_sample(SLOTS[1:2], runs[1:2], pos[1:2]) == ([want[0][1]], [want[1][1]])      # params[1]: a plain greedy sampler
    st.commit_multi([0])
    before = [st.slot_sampler_state(s) for s in SLOTS]
    greedy, nm = st.verify_multi(SLOTS, runs, pos)                            # the greedy verify neither reads nor advances the samplers
    assert (greedy, nm) == want
    st.commit_multi([m + 1 for m in nm])
    for s, b in zip(SLOTS, before):
        _smp_same(st.slot_sampler_state(s), b)


def test_refusals_and_the_pending_state():
    st, eng, orc, keep, d = build(kv_max=32)
    with pytest.raises(RuntimeError, match="no sequence slots"):
        st.verify_multi_sample([0], [[1, 2]], [0])
    with pytest.raises(RuntimeError, match="no sequence slots"):
        st.slot_sampler_state(0)
    st.create_slots(3, 24)
    st.fill_state_synthetic(d["kv_max"], seed=5)
    st.save_slot(1, 20)
    st.fill_state_synthetic(d["kv_max"], seed=6)
    st.save_slot(2, 10)
    st.set_slot_sampler(1, 2, 0.6, 50, 0.95, 0.5, 0x5EED)
    st.set_slot_sampler(2, 5, 0.0, 0, 1.0, 1.5, 3)
    state = lambda: (_slot_state(st, d, 1, 20), _slot_state(st, d, 2, 10))
    want, want_smp = state(), [st.slot_sampler_state(s) for s in (1, 2)]

    def unchanged():                                           # (load_slot inside: only while nothing is pending)
        for g, w in zip(state(), want):
            _same(g, w)

    def samplers_unchanged():
        for s, w in zip((1, 2), want_smp):
            _smp_same(st.slot_sampler_state(s), w)

    V = d["V"]
    refused = [
        (([1, 2], [[3], []], [20, 10]), "row 1"),                                           # a count of 0
        (([1], [[3] * (KR_VERIFY_MAX + 1)], [2]), "row 0"),                                 # a count of 17
        (([1] * 65, [[1] * 16] * 65, [0] * 65), "row 64"),                                  # T = 1040 > KR_EXTEND_MAX_TOKENS
        (([1, 1], [[3], [4]], [20, 21]), "row 1"),                                          # a slot named twice
        (([2, 1], [[3], [1, 2, 3, 4, 5]], [10, 20]), "row 1"),                              # last position == max_seq
        (([1], [[2, V, 3]], [20]), "row 0"),                                                # a draft token outside the vocabulary
    ]
    for args, row in refused:
        with pytest.raises(ValueError, match=row):
            st.verify_multi_sample(*args)
        unchanged(); samplers_unchanged()
    st.set_attention_mode(fast=True)                           # a tolerance bit
    try:
        with pytest.raises(RuntimeError, match="exact-mode only"):
            st.verify_multi_sample([1], [[2, 3]], [20])
    finally:
        st.set_attention_mode(False)
    unchanged(); samplers_unchanged()
    # the generate call checks its sampler arguments before the first pass
    with pytest.raises(ValueError, match="row 0: temperature"):
        st.generate_multi_lookup_sample([1], [2], [20], 2, temperature=[-1.0], rng_seeds=5)
    arr = lambda t, *xs: (t * len(xs))(*xs)
    i32 = lambda *xs: arr(C.c_int32, *xs)
    out, cnt = i32(0, 0), i32(0)
    temp, topk, topp, pen, seeds = arr(C.c_float, 0.7), arr(C.c_int, 5), arr(C.c_float, 0.9), arr(C.c_float, 0.0), arr(C.c_uint64, 5)
    for smp in ((None, topk, topp, pen, seeds), (temp, None, topp, pen, seeds), (temp, topk, topp, pen, None)):
        rc = st._lib.kr_decode_generate_multi_lookup_sample(st._h, 1, i32(1), None, None, i32(2), i32(20), 2, 4, 3, *smp, None, 0, out, cnt, None, None, None)
        assert rc != 0 and b"null sampler parameter array" in st._lib.kr_last_error()
    unchanged(); samplers_unchanged()

    ids, nm = st.verify_multi_sample([1, 2], [[2, 3, 4], [5, 6]], [20, 10])
    pending = [
        lambda: st.step_multi([1], [2], [20]),
        lambda: st.step_multi_sample([1], [2], [20]),
        lambda: st.extend_multi([1], [[2, 3]], [20]),
        lambda: st.generate_multi([1], [2], [20], 2, temperature=0.7, rng_seeds=5),
        lambda: st.generate_multi_lookup_sample([1], [2], [20], 2, temperature=0.7, rng_seeds=5),
        lambda: st.set_slot_sampler(1, 2, 0.8, 20, 0.9, 0.5, 7),
        lambda: st.slot_sampler_state(1),
        lambda: st.verify_multi([0], [[1]], [0]),
        lambda: st.verify_multi_sample([0], [[1]], [0]),
    ]
    for call in pending:
        with pytest.raises(RuntimeError, match="verify over slots is pending"):
            call()
    with pytest.raises(ValueError, match="row 0"):             # out of range: names its row, applies nothing, stays pending
        st.commit_multi([nm[0] + 2, 0])
    with pytest.raises(ValueError, match="row 1"):
        st.commit_multi([0, -1])
    with pytest.raises(RuntimeError, match="verify over slots is pending"):
        st.step_multi_sample([1], [2], [20])
    st.commit_multi([0, 0])
    unchanged(); samplers_unchanged()                          # every refused call and the dropped verify left slots and samplers as they were
    with pytest.raises(RuntimeError, match="no verify over slots is pending"):
        st.commit_multi([0, 0])
