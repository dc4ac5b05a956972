"""The "pass_few_rows" option and kr_decode_matmul_rows (docs/design/34-pass-few-rows.md): a multi-row pass of at most 16 token rows runs its projections on the
few-row streaming matvec (kr_rows_matvec.hip) and its INT4 / INT8 routed experts as the decode step's three launches.  No bit changes: the operator's row r is
matmul on row r; verify on the store's sequence equals decode_step token by token and the option-off call; every slot entry point gives what the same call gives
with the option off -- ids, logits, n_match, KV rows, conv / recurrent state, sampler state -- on flat and paged slots, with "multi_attn_exact_split" also set,
on FP16 and E4M3 caches, on native GGUF experts under "gguf_exact_pass", and on both sides of the row maximum.  There is no tolerance in this file: every
comparison is on ids and u32 / stored-row bit patterns.  Paged slots have pages of 32 positions -- kr_decode_slots_create_paged refuses smaller ones -- and the
rows and runs of every slot test lie on both sides of the page edges at 32 and 64."""
import functools

import numpy as np
import pytest

from tests.test_decode_gpu import MIXED, build
from tests.test_multi_mla_gpu import CFGS as MLA_CFGS, _build as build_mla, _same as mla_same, _snap as mla_snap
from tests.test_multi_seq_gpu import DV64, LA4
from tests.test_speculative_gpu import CFGS, _same, _snap

pytestmark = pytest.mark.gpu
F = np.float32
U = np.uint32
OPT, MAX, GROUP = "pass_few_rows", "pass_few_rows_max", "pass_few_rows_group"
ptr = lambda a: a.ctypes.data

_stores = []


@pytest.fixture(autouse=True)
def options_off_afterwards():
    yield
    for st in _stores:
        for o in (OPT, "multi_attn_exact_split", "gguf_exact_pass", GROUP):
            st.set_option(o, 0)
        st.set_option(MAX, 16)
        st.set_attention_mode(False)


def _bits(x):
    return np.ascontiguousarray(x, F).view(U).copy()


# ---- 1: the operator -----------------------------------------------------------------------------------------------------------------------------------------
KS, NS, ROWS = (128, 256, 384, 512), (1, 8, 344, 512), (1, 2, 3, 8, 15, 16)      # K = 128: one group, half a group pair; 384: an odd group count; N = 1: a partial tile


@functools.lru_cache(maxsize=None)
def _op_store():
    """one bare store holding every (bits, K, N) matrix of the operator cases, and the 16 input rows of every K"""
    from krasis_amd import CpuDecodeStore
    rng = np.random.default_rng(34)
    st = CpuDecodeStore(128, True, False)
    keep, wid = [], {}
    for bits in (4, 8):
        for K in KS + (4096,):
            for N in (NS if K != 4096 else (24,)):
                w = (rng.standard_normal((N, K)) * 0.05).astype(F); keep.append(w)
                wid[bits, K, N] = st.store_weight_f32(ptr(w), N, K, bits)
    xs = {K: (rng.standard_normal((16, K)) * rng.random((16, 1)) * 3.0).astype(F) for K in KS + (4096,)}
    _stores.append(st)
    return st, wid, xs, keep


def _row_by_row(st, w, x, N):
    out = np.empty((x.shape[0], N), F)
    for r in range(x.shape[0]):
        xr = np.ascontiguousarray(x[r]); y = np.empty(N, F)
        st.matmul(w, ptr(xr), ptr(y)); out[r] = y
    return out


def _rows(st, w, x, N):
    x = np.ascontiguousarray(x); y = np.full((x.shape[0], N), np.nan, F)
    st.matmul_rows(w, ptr(x), x.shape[0], ptr(y))
    return y


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("bits", [4, 8])
def test_matmul_rows_equals_matmul_row_by_row(bits, K):
    st, wid, xs, _ = _op_store()
    for N in NS:
        ref = _row_by_row(st, wid[bits, K, N], xs[K], N)      # once per matrix, shared by every row count
        for R in ROWS:
            got = _rows(st, wid[bits, K, N], xs[K][:R], N)
            assert np.array_equal(_bits(got), _bits(ref[:R])), (bits, K, N, R)


@pytest.mark.parametrize("group", [0, 1, 3, 4, 8, 16])
@pytest.mark.parametrize("bits", [4, 8])
def test_matmul_rows_k4096_row_groups(bits, group):
    """K = 4096: 16 images exceed 64 KiB (INT4: 146 KiB, INT8: 274 KiB), so the launch takes the LDS opt-in and, for INT8 or a forced group, several row groups on
    gridDim.y; every forced row-group size gives the same bits"""
    st, wid, xs, _ = _op_store()
    K, N = 4096, 24
    ref = _row_by_row(st, wid[bits, K, N], xs[K], N)
    st.set_option(GROUP, group)
    for R in (16, 15, 5):
        assert np.array_equal(_bits(_rows(st, wid[bits, K, N], xs[K][:R], N)), _bits(ref[:R])), (bits, group, R)


@pytest.mark.parametrize("bits", [4, 8])
def test_matmul_rows_zero_rows_and_extreme_values(bits):
    """rows that are all zero (scale 1, every digit 0) between ordinary ones, and a row whose groups hold the quantiser's extremes: +-max of the group (digits
    +-32767), the largest finite f32, values that round to digit 0 beside them, one non-zero value in a group"""
    st, wid, xs, _ = _op_store()
    K, N = 384, 344
    x = xs[K][:8].copy()
    x[1] = 0.0; x[6] = 0.0
    ext = np.zeros(K, F)
    ext[0:128:2] = 3.0; ext[1:128:2] = -3.0; ext[5] = 1e-30                        # +-32767 in every chunk, one value far below half a digit
    ext[128:256] = np.float32(3.4028235e38) * np.where(np.arange(128) % 3 == 0, 1, -1); ext[130] = 1.0
    ext[300] = -7.25                                                               # a group with one non-zero value
    x[3] = ext
    ref = _row_by_row(st, wid[bits, K, N], x, N)
    got = _rows(st, wid[bits, K, N], x, N)
    assert np.array_equal(_bits(got), _bits(ref))
    assert not np.any(_bits(got[1])) and not np.any(_bits(got[6]))                 # +0.0 exactly


def test_matmul_rows_refuses_bad_row_counts():
    st, wid, xs, _ = _op_store()
    x = xs[128]; y = np.empty((16, 8), F)
    for n in (0, 17, -1):
        with pytest.raises(ValueError, match="n_rows"):
            st.matmul_rows(wid[4, 128, 8], ptr(x), n, ptr(y))
    with pytest.raises(ValueError, match="out of range"):
        st.matmul_rows(10 ** 6, ptr(x), 2, ptr(y))


# ---- 2: verify on the store's own sequence -------------------------------------------------------------------------------------------------------------------
def _verify_on_off(st, reset, snap, same, V, first=11, start=5, kv_extra=0):
    """runs of 1, 2, 5 and 16 tokens whose drafts are the greedy continuation, and a run of 5 with a wrong draft.  Yardstick: decode_step token by token.  Option
    on and off: greedy ids, n_match, and after commit(k) for every k the logits (row k - 1 of the pass), the last token and the state"""
    reset()
    T = st.generate_batch(first, start, 16)
    assert len(T) == 16
    for n, wrong in ((1, None), (2, None), (5, None), (16, None), (5, 2)):
        toks = [first] + T[:n - 1]
        if wrong is not None:
            toks[wrong] = (toks[wrong] + 1) % V
        n_ok = n if wrong is None else wrong
        reset()
        ref = []
        for i, t in enumerate(toks[:n_ok]):
            st.decode_step(t, start + i)
            ref.append((_bits(st.read_logits()), st.last_token(), snap(start + i + 1)))
        res = {}
        for on in (0, 1):
            st.set_option(OPT, on)
            out = []
            for k in range(1, n_ok + 1):
                reset()
                greedy, m = st.verify(toks, start)
                assert m == n_ok - 1 and greedy[:n_ok] == T[:n_ok], (n, wrong, on, greedy, m)
                st.commit(k)
                lg, tok = _bits(st.read_logits()), st.last_token()
                assert np.array_equal(lg, ref[k - 1][0]) and tok == ref[k - 1][1], ("decode_step", n, wrong, on, k)
                same(snap(start + k), ref[k - 1][2])
                out.append((list(greedy), m, lg))
            res[on] = out
            st.set_option(OPT, 0)
        for a, b in zip(res[0], res[1]):
            assert a[0] == b[0] and a[1] == b[1] and np.array_equal(a[2], b[2]), (n, wrong)


WIDE_SHARED = dict(dims=(256, 512, 16, 4, 128, 384), seed=3)      # the shared expert three times as wide as the routed ones
K10 = dict(dims=(256, 512, 512, 10, 128, 128), seed=6)           # 512 experts, k = 10


@pytest.mark.parametrize("cfg", CFGS + [MIXED, WIDE_SHARED, K10], ids=lambda c: "-".join(sorted(c)) or "default")
def test_verify_equals_decode_step_and_option_off(cfg):
    st, eng, orc, keep, d = build(**cfg)
    _stores.append(st)
    _verify_on_off(st, d["reset"], lambda upto: _snap(st, d, upto), _same, d["V"])


def test_verify_mla_lora():
    st, eng, keep, d = build_mla(kv_max=32, **MLA_CFGS[1])
    assert MLA_CFGS[1].get("lora")
    _stores.append(st)
    _verify_on_off(st, lambda: st.reset_decode_state(d["kv_max"]), lambda upto: mla_snap(st, d, upto), mla_same, d["V"], start=0)


# ---- 3: slots: every call equals the same call with the option off -------------------------------------------------------------------------------------------
KV_MAX = 96
PAGE = 32                                                                   # the smallest page kr_decode_slots_create_paged accepts
SLOTS = [5, 12, 0, 7, 2, 14, 9, 3, 11, 6, 1, 13, 4, 10, 8, 15, 16]          # slot numbers do not follow the rows
VARIANTS = [dict(), dict(paged=True), dict(split=True), dict(fp8=True), dict(paged=True, split=True, fp8=True)]


@functools.lru_cache(maxsize=None)
def _model(fp8=False, mla=False):
    if mla:
        st, eng, keep, d = build_mla(fp8, kv_max=KV_MAX, **MLA_CFGS[1])
    else:
        st, eng, orc, keep, d = build(seed=3, kv_max=KV_MAX)
        if fp8:
            st.set_kv_dtype(True); d["fp8"] = True
        keep = (eng, orc, keep)
    _stores.append(st)
    seq = tuple(int(x) for x in np.random.default_rng(7 + fp8 + 2 * mla).integers(0, d["V"], KV_MAX))
    return st, keep, d, seq


def _fill(st, d, seq, want):
    """want = [(slot, n)]: the first n tokens of seq by the store's prompt pass (option off), one pass per slot: recurrent state belongs to its prefix"""
    for s, n in want:
        st.reset_decode_state(d["kv_max"])
        if n:
            st.prefill(list(seq[:n]), 0)
        st.save_slot(s, n)


def _slot_state(st, d, slot, upto, mla=False):
    st.reset_decode_state(d["kv_max"])
    st.load_slot(slot, upto)
    return mla_snap(st, d, upto) if mla else _snap(st, d, upto)


def _create(st, n, paged=False, **_):
    if paged:
        st.create_slots(n, KV_MAX, page_tokens=PAGE, n_pages=n * (KV_MAX // PAGE))
    else:
        st.create_slots(n, KV_MAX)


def _off_on(st, scenario, split=False, max_rows=16, **_):
    """scenario() -> (ids, logits, states, extra) on slots it creates and fills itself (filling always with the option off), once with the option off, once on"""
    out = []
    for on in (0, 1):
        st.set_option("multi_attn_exact_split", 1 if split else 0)
        if split:
            st.set_option("multi_attn_exact_split_min", 1)
        st.set_option(MAX, max_rows)
        out.append(scenario(lambda: st.set_option(OPT, on)))
        st.set_option(OPT, 0); st.set_option("multi_attn_exact_split", 0); st.set_option(MAX, 16)
    return out


def _equal(a, b, where, mla=False):
    assert [int(x) for x in a[0]] == [int(x) for x in b[0]], ("ids", where)
    assert np.array_equal(_bits(a[1]), _bits(b[1])), ("logits", where)
    assert len(a[2]) == len(b[2])
    for x, y in zip(a[2], b[2]):
        (mla_same if mla else _same)(x, y)
    assert len(a[3]) == len(b[3])
    for x, y in zip(a[3], b[3]):
        assert np.array_equal(x, y), ("sampler state", where)


# row 0 at position 0 (an empty slot), the others behind prefixes of unlike lengths: the last row of a page, the first of the next, and rows beside them
POSN = [0, 31, 32, 63, 64, 30, 5, 70, 12, 33, 1, 62, 47, 20, 65, 8, 40]


def _positions(B):
    return POSN[:B]


@pytest.mark.parametrize("var", VARIANTS, ids=lambda v: "-".join(sorted(v)) or "flat")
@pytest.mark.parametrize("B", [1, 2, 7, 16])
def test_step_multi(B, var):
    st, _, d, seq = _model(var.get("fp8", False))
    pos, slots = _positions(B), SLOTS[:B]
    took = []      # not vacuous: both passes took the few-row form in the on-leg, none in the off-leg (multi_path_counts)

    def scenario(arm):
        _create(st, 17, **var)
        _fill(st, d, seq, list(zip(slots, pos)))
        arm()
        st.multi_path_counts(reset=True)
        ids, lg = st.step_multi(slots, [seq[p] for p in pos], pos, logits=True)
        ids2, lg2 = st.step_multi(slots, list(ids), [p + 1 for p in pos], logits=True)      # a second step over what the first appended
        took.append(st.multi_path_counts()["few"])
        st.set_option(OPT, 0)
        return list(ids) + list(ids2), np.concatenate([lg, lg2]), [_slot_state(st, d, s, p + 2) for s, p in zip(slots, pos)], []

    off, on = _off_on(st, scenario, **var)
    assert took == [0, 2], ("few", took)
    _equal(on, off, ("step_multi", B, var))


@pytest.mark.parametrize("var", VARIANTS, ids=lambda v: "-".join(sorted(v)) or "flat")
def test_extend_multi_sixteen_rows(var):
    st, _, d, seq = _model(var.get("fp8", False))
    counts, pos, slots = [1, 9, 5, 1], [31, 28, 60, 7], SLOTS[:4]      # runs across the page edges at 32 and 64

    def scenario(arm):
        _create(st, 17, **var)
        _fill(st, d, seq, list(zip(slots, pos)))
        arm()
        ids, lg = st.extend_multi(slots, [list(seq[p:p + c]) for p, c in zip(pos, counts)], pos, logits=True)
        st.set_option(OPT, 0)
        return ids, lg, [_slot_state(st, d, s, p + c) for s, p, c in zip(slots, pos, counts)], []

    off, on = _off_on(st, scenario, **var)
    _equal(on, off, ("extend_multi", var))


@pytest.mark.parametrize("var", VARIANTS, ids=lambda v: "-".join(sorted(v)) or "flat")
def test_verify_multi_and_commit(var):
    """runs of 5, 5, 3 and 3 tokens (16 rows).  First pass: drafts from the random sequence (rejected), committed as nothing.  Second: drafts = the greedy ids of
    a pass of their own, one of them made wrong; committed at n_match + 1"""
    st, _, d, seq = _model(var.get("fp8", False))
    counts, pos, slots = [5, 5, 3, 3], [30, 0, 62, 20], SLOTS[:4]      # two runs across a page edge

    def scenario(arm):
        _create(st, 17, **var)
        _fill(st, d, seq, list(zip(slots, pos)))
        arm()
        g1, nm1 = st.verify_multi(slots, [list(seq[p:p + c]) for p, c in zip(pos, counts)], pos)
        st.commit_multi([0] * 4)
        runs = [[seq[p]] for p in pos]
        for _ in range(4):                                   # the greedy continuation, one token further per pass
            g, _nm = st.verify_multi(slots, runs, pos)
            st.commit_multi([0] * 4)
            runs = [[seq[p]] + list(row[:c - 1]) for p, row, c in zip(pos, g, counts)]
        runs = [r[:c] for r, c in zip(runs, counts)]
        runs[1][3] = (runs[1][3] + 1) % d["V"]               # a rejected draft among matching ones
        g2, nm2 = st.verify_multi(slots, runs, pos)
        assert list(nm2) == [4, 2, 2, 2], list(nm2)
        keep = [m + 1 for m in nm2]
        st.commit_multi(keep)
        st.set_option(OPT, 0)
        ids = [x for row, m in zip(g1, nm1) for x in row[:m + 1]] + list(nm1) + [x for row, m in zip(g2, nm2) for x in row[:m + 1]] + list(nm2)
        return ids, np.zeros(1, F), [_slot_state(st, d, s, p + k) for s, p, k in zip(slots, pos, keep)], []

    off, on = _off_on(st, scenario, **var)
    _equal(on, off, ("verify_multi", var))


@pytest.mark.parametrize("var", VARIANTS, ids=lambda v: "-".join(sorted(v)) or "flat")
def test_step_multi_sample(var):
    st, _, d, seq = _model(var.get("fp8", False))
    B = 7
    pos, slots = _positions(B), SLOTS[:B]

    def scenario(arm):
        _create(st, 17, **var)
        _fill(st, d, seq, list(zip(slots, pos)))
        for i, s in enumerate(slots):
            st.set_slot_sampler(s, seq[pos[i]], 0.8, 40, 0.95, 0.5, 100 + i)
        arm()
        ids, lg = st.step_multi_sample(slots, [seq[p] for p in pos], pos, logits=True)
        ids2, lg2 = st.step_multi_sample(slots, list(ids), [p + 1 for p in pos], logits=True)
        st.set_option(OPT, 0)
        extra = []
        for s in slots:
            seen, rng_state = st.slot_sampler_state(s)
            extra += [np.asarray(seen), np.asarray([rng_state], np.uint64)]
        return list(ids) + list(ids2), np.concatenate([lg, lg2]), [_slot_state(st, d, s, p + 2) for s, p in zip(slots, pos)], extra

    off, on = _off_on(st, scenario, **var)
    _equal(on, off, ("step_multi_sample", var))


@pytest.mark.parametrize("fp8", [False, True])
def test_step_and_extend_multi_mla(fp8):
    """MLA layers with the LoRA query path (kv_a, q_a, q_b, o on the few-row kernel), a dense MLP layer and a shared expert twice the routed width"""
    st, _, d, seq = _model(fp8, mla=True)
    counts, pos, slots = [1, 9, 5, 1], [3, 0, 10, 7], SLOTS[:4]

    def scenario(arm):
        st.create_slots(17, KV_MAX)
        _fill(st, d, seq, list(zip(slots, pos)))
        arm()
        ids, lg = st.extend_multi(slots, [list(seq[p:p + c]) for p, c in zip(pos, counts)], pos, logits=True)
        ids2, lg2 = st.step_multi(slots, list(ids), [p + c for p, c in zip(pos, counts)], logits=True)
        st.set_option(OPT, 0)
        return list(ids) + list(ids2), np.concatenate([lg, lg2]), [_slot_state(st, d, s, p + c + 1, mla=True) for s, p, c in zip(slots, pos, counts)], []

    off, on = _off_on(st, scenario)
    _equal(on, off, ("mla", fp8), mla=True)


@pytest.mark.parametrize("cfg", [LA4, DV64, MIXED], ids=["la4", "dv64", "mixed"])
def test_step_multi_other_geometries(cfg):
    """linear attention alone with four value heads per key head, dv < dk, and the mixed 4 / 8-bit store (every grouped launch falls back to one per matrix)"""
    st, eng, orc, keep, d = build(kv_max=KV_MAX, **cfg)
    _stores.append(st)
    seq = [int(x) for x in np.random.default_rng(11).integers(0, d["V"], KV_MAX)]
    B = 5
    pos, slots = _positions(B), SLOTS[:B]

    def fill():
        for s, n in zip(slots, pos):
            st.reset_decode_state(d["kv_max"])
            for i, t in enumerate(seq[:n]):      # decode_step: the prompt pass refuses dv < dk
                st.decode_step(t, i)
            st.save_slot(s, n)

    def scenario(arm):
        st.create_slots(17, KV_MAX)
        fill()
        arm()
        ids, lg = st.step_multi(slots, [seq[p] for p in pos], pos, logits=True)
        st.set_option(OPT, 0)
        return ids, lg, [_slot_state(st, d, s, p + 1) for s, p in zip(slots, pos)], []

    off, on = _off_on(st, scenario)
    _equal(on, off, ("geometry", sorted(cfg)))


# ---- 4: the row maximum: the fallback gives the same bits (tests/test_pass_few_rows.py proves which form a pass takes) ----------------------------------------
@pytest.mark.parametrize("T,max_rows", [(17, 16), (5, 4), (4, 4), (16, 16)])
def test_row_maximum_boundary(T, max_rows):
    st, _, d, seq = _model(False)
    pos, slots = [(3 * i) % 19 for i in range(T)], SLOTS[:T]

    def scenario(arm):
        _create(st, 17)
        _fill(st, d, seq, list(zip(slots, pos)))
        arm()
        ids, lg = st.step_multi(slots, [seq[p] for p in pos], pos, logits=True)
        st.set_option(OPT, 0)
        return ids, lg, [_slot_state(st, d, s, p + 1) for s, p in zip(slots, pos)], []

    off, on = _off_on(st, scenario, max_rows=max_rows)
    _equal(on, off, ("boundary", T, max_rows))


# ---- 5: native GGUF experts ----------------------------------------------------------------------------------------------------------------------------------
def test_gguf_exact_pass_verify():
    """a store whose routed experts are native GGUF blocks, under "gguf_exact_pass": the routed experts keep their pass, the dense matrices switch; verify of 5"""
    st, eng, orc, keep, d = build(gguf=True, dims=(256, 512, 8, 3, 256, 128), seed=11)
    st.set_option("gguf_exact_pass", 1)
    _verify_on_off(st, d["reset"], lambda upto: _snap(st, d, upto), _same, d["V"])      # runs of 1, 2, 5 and 16 tokens; every row's logits through commit(k)
    st.set_option("gguf_exact_pass", 0)


# ---- 6: the options -------------------------------------------------------------------------------------------------------------------------------------------
def test_maximum_out_of_range_is_a_value_error():
    st, _, d, seq = _model(False)
    for v in (0, 17, -3):
        with pytest.raises(ValueError) as e:
            st.set_option(MAX, v)
        assert MAX in str(e.value), str(e.value)
    for v in (-1, 17):
        with pytest.raises(ValueError) as e:
            st.set_option(GROUP, v)
        assert GROUP in str(e.value), str(e.value)
    for v in (1, 16):
        st.set_option(MAX, v)


def test_gemm_fast_prefill_keeps_its_bits():
    """mode bit 2 (KR_GEMM_FAST): the tolerance GEMMs keep a prompt pass of 8 tokens whatever the option says"""
    st, _, d, seq = _model(False)
    res = []
    for on in (0, 1):
        st.set_attention_mode(False, gemm_fast=True)
        st.set_option(OPT, on)
        st.reset_decode_state(d["kv_max"])
        tok = st.prefill(list(seq[:8]), 0)
        res.append((tok, _bits(st.read_logits()), _snap(st, d, 8)))
        st.set_option(OPT, 0); st.set_attention_mode(False)
    assert res[0][0] == res[1][0] and np.array_equal(res[0][1], res[1][1])
    _same(res[0][2], res[1][2])


def test_exact_prefill_of_few_tokens_equals_option_off_and_decode_step():
    """kr_decode_prefill is a multi-row pass too: 8 tokens, option on == off == decode_step token by token"""
    st, _, d, seq = _model(False)
    st.reset_decode_state(d["kv_max"])
    for i, t in enumerate(seq[:8]):
        st.decode_step(t, i)
    ref = (st.last_token(), _bits(st.read_logits()), _snap(st, d, 8))
    for on in (0, 1):
        st.set_option(OPT, on)
        st.reset_decode_state(d["kv_max"])
        tok = st.prefill(list(seq[:8]), 0)
        assert tok == ref[0] and np.array_equal(_bits(st.read_logits()), ref[1]), on
        _same(_snap(st, d, 8), ref[2])
        st.set_option(OPT, 0)
