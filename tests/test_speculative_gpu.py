"""Exact speculative greedy decoding (kr_decode_verify / kr_decode_commit / kr_decode_generate_lookup): a verify pass over [last token, drafts]
followed by a commit of n_keep tokens leaves the store BIT-IDENTICAL to n_keep decode steps (logits, last token, conv and recurrent states, KV rows
below the committed length), and generate_lookup returns exactly generate_batch's greedy stream.  KV rows at or past the committed length are
unspecified (the next pass overwrites them) and are not compared."""
import ctypes as C

import numpy as np
import pytest

from tests.test_decode_gpu import build

pytestmark = pytest.mark.gpu
F = np.float32


def _snap(st, d, upto):
    """conv + recurrent states of every linear-attention layer (u32 bits), KV rows [0, upto) of every GQA layer"""
    out = []
    for li, kind in enumerate(d["kinds"]):
        if kind == "la":
            cs = np.empty(d["conv_dim"] * 4, F); rs = np.empty(d["nv"] * d["dk"] * d["dv"], F)
            st.get_decode_state(li, None, None, cs, rs); out.append(("la", li, cs.view(np.uint32).copy(), rs.view(np.uint32).copy()))
        else:
            esz = np.uint8 if d.get("fp8") else np.uint16
            kc = np.empty((d["kv_max"], d["nkv"] * d["hd"]), esz); vc = np.empty_like(kc)
            st.get_decode_state(li, kc, vc, None, None); out.append(("kv", li, kc[:upto].copy(), vc[:upto].copy()))
    return out


def _same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert x[0] == y[0] and x[1] == y[1]
        assert np.array_equal(x[2], y[2]), (x[0], x[1], "conv" if x[0] == "la" else "k")
        assert np.array_equal(x[3], y[3]), (x[0], x[1], "recur" if x[0] == "la" else "v")


def _sequential(st, d, toks, start):
    """decode_step over toks from the current state; the store's (logits bits, last token, snapshot) after each step"""
    out = []
    for i, t in enumerate(toks):
        st.decode_step(t, start + i)
        out.append((st.read_logits().view(np.uint32).copy(), st.last_token(), _snap(st, d, start + i + 1)))
    return out


def _check_state(st, d, ref, n_keep, start):
    lg, tok, snap = ref[n_keep - 1]
    assert np.array_equal(st.read_logits().view(np.uint32), lg)
    assert st.last_token() == tok
    _same(_snap(st, d, start + n_keep), snap)


CFGS = [dict(), dict(norm_bias_one=False, scoring=0, rsf=2.5), dict(with_dense=True), dict(wbits=8, with_dense=True), dict(la_dkdv=(64, 64), seed=4)]


@pytest.mark.parametrize("cfg", CFGS)
def test_all_drafts_right_commit_equals_sequential_decode(cfg):
    st, eng, orc, keep, d = build(**cfg)
    first = 11
    for start in (0, 5):
        d["reset"]()
        T = st.generate_batch(first, start, 16)
        assert len(T) == 16
        for n in (1, 2, 5, 9, 16):
            toks = [first] + T[:n - 1]
            d["reset"]()
            ref = _sequential(st, d, toks + [T[n - 1]], start)        # n steps + the step after them
            d["reset"]()
            greedy, m = st.verify(toks, start)
            assert greedy == T[:n] and m == n - 1, (n, start, greedy, T[:n], m)
            st.commit(n)
            _check_state(st, d, ref, n, start)
            st.decode_step(T[n - 1], start + n)                        # and decoding continues seamlessly
            _check_state(st, d, ref, n + 1, start)


@pytest.mark.parametrize("cfg", [dict(), dict(la_dkdv=(64, 64), seed=4), dict(with_dense=True)])
def test_partial_acceptance_rolls_back_exactly(cfg):
    st, eng, orc, keep, d = build(**cfg)
    first, start, n = 7, 5, 9
    d["reset"]()
    T = st.generate_batch(first, start, 20)
    d["reset"]()
    ref = _sequential(st, d, [first] + T[:n - 1], start)
    for j in range(1, n):                 # draft j (tokens[j]) is wrong: drafts 1 .. j-1 match, n_keep = j (j < 4: the conv slots mix snapshot and kept inputs)
        toks = [first] + T[:n - 1]
        toks[j] = (toks[j] + 1) % d["V"]
        d["reset"]()
        greedy, m = st.verify(toks, start)
        assert m == j - 1, (j, m)
        assert greedy[:j] == T[:j]
        st.commit(j)
        _check_state(st, d, ref, j, start)
        assert st.generate_batch(T[j - 1], start + j, n - j) == T[j:n]


def test_truncated_commit():
    st, eng, orc, keep, d = build(seed=2)
    first, start, n = 3, 5, 12
    d["reset"]()
    T = st.generate_batch(first, start, 20)
    d["reset"]()
    ref = _sequential(st, d, [first] + T[:n - 1], start)
    for n_keep in (1, 2, 3, 6, n - 1):
        d["reset"]()
        greedy, m = st.verify([first] + T[:n - 1], start)
        assert m == n - 1
        st.commit(n_keep)                  # fewer than the verify accepted
        _check_state(st, d, ref, n_keep, start)
        assert st.generate_batch(T[n_keep - 1], start + n_keep, 4) == T[n_keep:n_keep + 4]


def _state_after(st, d, upto):
    return st.last_token(), st.read_logits().view(np.uint32).copy(), _snap(st, d, upto)


def _compare_lookup(st, d, reset, first, start, max_tokens, context, max_draft, ngram_max, stop_ids=()):
    reset()
    ref = st.generate_batch(first, start, max_tokens, stop_ids=stop_ids)
    ref_state = _state_after(st, d, start + len(ref))
    reset()
    out = st.generate_lookup(first, start, max_tokens, context=context, max_draft=max_draft, ngram_max=ngram_max, stop_ids=stop_ids)
    assert out == ref, (out, ref)
    tok, lg, snap = _state_after(st, d, start + len(out))
    assert tok == ref_state[0] and np.array_equal(lg, ref_state[1])
    _same(snap, ref_state[2])
    return ref, st.last_lookup_stats


@pytest.mark.parametrize("cfg", [dict(), dict(with_dense=True, seed=9), dict(la_dkdv=(64, 64), seed=4)])
@pytest.mark.parametrize("max_draft,ngram_max", [(1, 1), (4, 3), (15, 3), (15, 1)])
def test_generate_lookup_equals_generate_batch(cfg, max_draft, ngram_max):
    st, eng, orc, keep, d = build(**cfg)
    reset = lambda: st.reset_decode_state(d["kv_max"])
    first, start, M = 5, 3, 24
    rng = np.random.default_rng(max_draft * 7 + ngram_max)
    ctx = [int(x) for x in rng.integers(0, d["V"], 40)]
    _compare_lookup(st, d, reset, first, start, M, ctx, max_draft, ngram_max)             # random context: few drafts accepted
    reset()
    T = st.generate_batch(first, start, M)
    T_out, stats = _compare_lookup(st, d, reset, first, start, M, [first] + T, max_draft, ngram_max)     # the context repeats the greedy stream
    assert stats["accepted"] > 0
    if max_draft >= 4 and ngram_max == 3:
        assert stats["passes"] <= M // 2, stats
    _compare_lookup(st, d, reset, first, start, 7, [first] + T, max_draft, ngram_max)      # max_tokens cuts an accepted run
    stop = T[5]
    _compare_lookup(st, d, reset, first, start, M, [first] + T, max_draft, ngram_max, stop_ids=(stop, d["V"] + 3))   # a stop id inside an accepted run
    _compare_lookup(st, d, reset, first, start, M, [first] + T, 0, ngram_max)               # max_draft 0: the plain loop


def test_generate_lookup_passes_follow_the_drafting_rule():
    """the loop's incremental n-gram index proposes kr_lookup_draft's drafts: passes / accepted predicted from the rule and the known stream"""
    from krasis_amd.decode_store import lookup_draft
    st, eng, orc, keep, d = build(seed=13)
    reset = lambda: st.reset_decode_state(d["kv_max"])
    first, start, M = 2, 0, 28
    reset()
    T = st.generate_batch(first, start, M)
    for ctx, md, ng in (([first] + T[:10] + [1, 2, 3] + T, 6, 3), ([9, 9] + T[::2], 5, 2), ([first] + T, 15, 1)):
        hist, n, passes, acc = list(ctx) + [first], 0, 0, 0
        while n < M:
            dr = lookup_draft(hist, ng, md)[:max(0, M - n - 1)]
            dr = dr[:max(0, d["kv_max"] - (start + n) - 1)]
            passes += 1
            m = 0
            while m < len(dr) and dr[m] == T[n + m]:
                m += 1
            acc += m
            hist += T[n:n + m + 1]; n += m + 1
        reset()
        assert st.generate_lookup(first, start, M, context=ctx, max_draft=md, ngram_max=ng) == T
        assert st.last_lookup_stats == {"passes": passes, "accepted": acc}, (st.last_lookup_stats, passes, acc)


def _raw_generate(st, lookup, first, start, max_tokens, ctx=(), max_draft=8):
    """both loops through the C ABI directly: the tokens written before an error are visible"""
    lib = st._lib
    out = (C.c_int * max_tokens)(*([-1] * max_tokens)); n = C.c_int(-1); stops = (C.c_int * 1)()
    if lookup:
        cx = (C.c_int32 * max(len(ctx), 1))(*ctx); p = C.c_int(); a = C.c_int()
        rc = lib.kr_decode_generate_lookup(st._h, cx, len(ctx), first, start, max_tokens, max_draft, 3, stops, 0, out, C.byref(n), C.byref(p), C.byref(a), None)
    else:
        rc = lib.kr_decode_generate_greedy(st._h, first, start, max_tokens, stops, 0, out, C.byref(n), None)
    return rc, lib.kr_last_error().decode() if rc else "", list(out), n.value


def test_generate_lookup_at_the_cache_boundary():
    st, eng, orc, keep, d = build(seed=5)
    kv = d["kv_max"]
    reset = lambda: st.reset_decode_state(kv)
    first, start = 4, kv - 12
    reset()
    T = st.generate_batch(first, start, 12)            # fills the cache exactly
    for max_tokens in (12, 20):                        # 20: the step at position kv fails, after 12 tokens
        reset(); ref = _raw_generate(st, False, first, start, max_tokens)
        ref_state = _state_after(st, d, kv)
        reset(); got = _raw_generate(st, True, first, start, max_tokens, ctx=[first] + T + T)
        assert got == ref, (got, ref)
        tok, lg, snap = _state_after(st, d, kv)
        assert tok == ref_state[0] and np.array_equal(lg, ref_state[1])
        _same(snap, ref_state[2])
    assert ref[0] != 0 and "kv_max_seq" in ref[1]


def test_generate_lookup_fp8_kv():
    st, eng, orc, keep, d = build(seed=6)
    st.set_kv_dtype(True); d["fp8"] = True
    reset = lambda: st.reset_decode_state(d["kv_max"])
    reset()
    T = st.generate_batch(8, 2, 20)
    _compare_lookup(st, d, reset, 8, 2, 20, [8] + T, 8, 3)
    _compare_lookup(st, d, reset, 8, 2, 20, [1, 2, 3, 4], 8, 3)


@pytest.mark.parametrize("cfg", [dict(), dict(lora=True, seed=2)])
def test_generate_lookup_mla(cfg):
    from tests.test_mla_gpu import build as build_mla
    st, eng, orc, keep, d = build_mla(**cfg)
    kv = d["kv_max"]

    def state():
        out = [st.last_token(), st.read_logits().view(np.uint32).copy()]
        for li in range(d["nL"]):
            ck = np.empty((kv, d["klr"]), np.uint16); kp = np.empty((kv, d["rd"]), np.uint16)
            st.get_decode_state(li, ck, kp, None, None); out.append((ck, kp))
        return out
    first, start, M = 9, 2, 16
    st.reset_decode_state(kv)
    T = st.generate_batch(first, start, M)
    ref = state()
    for ctx, md in (([first] + T, 15), ([first] + T, 4), ([5, 6, 7], 8)):
        st.reset_decode_state(kv)
        assert st.generate_lookup(first, start, M, context=ctx, max_draft=md) == T
        got = state()
        assert got[0] == ref[0] and np.array_equal(got[1], ref[1])
        for (a, b), (c, e) in zip(got[2:], ref[2:]):
            assert np.array_equal(a[:start + M], c[:start + M]) and np.array_equal(b[:start + M], e[:start + M])
    st.reset_decode_state(kv)
    st.generate_lookup(first, start, M, context=[first] + T, max_draft=15)
    assert st.last_lookup_stats["passes"] <= M // 2 and st.last_lookup_stats["accepted"] > 0


def test_production_widths():
    """QCN widths: hidden 2048, 32 value heads of 128 (16 key heads), vocab 151 936 -- the accept kernel over full rows and the rollback of full-size states"""
    import bench
    q = bench.QCN
    eng, st, keep = bench.build_qcn(0, 0, 4)
    kv = q["kv_max_seq"]
    reset = lambda: st.fill_state_synthetic(kv, seed=4242)
    nk, nv, dk, dv = q["nk"], q["nv"], q["dk"], q["dv"]
    d = dict(kinds=["gqa" if bench.is_gqa(l) else "la" for l in range(4)], conv_dim=2 * nk * dk + nv * dv, nv=nv, dk=dk, dv=dv, kv_max=kv, nkv=q["nkv"], hd=q["hd"])
    first, start, n = 1, 100, 9
    reset()
    T = st.generate_batch(first, start, n)
    reset()
    ref = _sequential(st, d, [first] + T[:n - 1], start)
    for j in (3, n):
        toks = [first] + T[:n - 1]
        if j < n:
            toks[j] = (toks[j] + 17) % q["vocab"]
        reset()
        greedy, m = st.verify(toks, start)
        assert greedy[:j] == T[:j] and m == j - 1
        st.commit(j)
        _check_state(st, d, ref, j, start)


def test_refusals_and_argument_errors():
    st, eng, orc, keep, d = build(seed=8)
    d["reset"]()
    with pytest.raises(RuntimeError, match="without a pending"):
        st.commit(1)
    with pytest.raises(ValueError):
        st.verify([], 5)
    with pytest.raises(ValueError):
        st.verify([1] * 17, 5)
    with pytest.raises(ValueError, match="out of range"):
        st.verify([1, d["V"]], 5)
    with pytest.raises(ValueError):
        st.verify([1, 2, 3], d["kv_max"] - 2)              # does not fit the cache
    with pytest.raises(ValueError):
        st.verify([1, 2], -1)
    with pytest.raises(ValueError):
        st.generate_lookup(1, 5, 4, max_draft=16)
    with pytest.raises(ValueError):
        st.generate_lookup(1, 5, 4, ngram_max=0)
    with pytest.raises(ValueError):
        st.generate_lookup(1, 5, 4, context=[d["V"]])
    greedy, m = st.verify([1, 2, 3], 5)
    with pytest.raises(ValueError, match="n_keep"):
        st.commit(m + 2)
    with pytest.raises(ValueError, match="n_keep"):
        st.commit(0)
    for call in (lambda: st.decode_step(1, 5), lambda: st.prefill([1, 2], 5), lambda: st.verify([1], 5), lambda: st.generate_batch(1, 5, 2),
                 lambda: st.generate_lookup(1, 5, 2), lambda: st.prefill_nll([1, 2], 5)):
        with pytest.raises(RuntimeError, match="pending"):
            call()
    st.commit(1)                                            # still pending after the refused calls: one commit goes through
    st.decode_step(greedy[0], 6)
    st.verify([1, 2], 5)
    st.reset_decode_state(d["kv_max"])                      # a new state discards the pending verify
    st.decode_step(1, 0)
    st.verify([1, 2], 1)
    d["reset"]()                                            # set_decode_state too
    st.generate_batch(1, 5, 2)
    for mode in (dict(fast=True), dict(fast=False, gemm_fast=True), dict(fast=False, decode_fast=True)):
        st.set_attention_mode(**mode)
        with pytest.raises(RuntimeError, match="exact-mode only"):
            st.verify([1, 2], 5)
        with pytest.raises(RuntimeError, match="exact-mode only"):
            st.generate_lookup(1, 5, 4)
    st.set_attention_mode(False)
    st.verify([1, 2], 5); st.commit(1)


def test_native_gguf_moe_is_refused():
    st, eng, orc, keep, d = build(dims=(256, 512, 16, 4, 128, 128), gguf=True, seed=11)
    with pytest.raises(RuntimeError, match="GGUF"):
        st.verify([1, 2], 5)
    with pytest.raises(RuntimeError, match="GGUF"):
        st.generate_lookup(1, 5, 4, context=[1, 2])
