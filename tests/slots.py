"""Shared scaffolding of the GPU tests of the batched pass over device slots (not collected: the name is no test_*.py).

A "kind" is one of the two test models with its single-sequence reference helpers: Gqa, the hybrid linear-attention + GQA model of tests/test_decode_gpu.py, and
Mla, the MLA model of tests/test_mla_gpu.py.  A kind builds a store, brings the store's own sequence to a prompt, runs decode_step alone as the reference, and
snapshots and compares the per-layer state.  Every comparison offered here is on ids and on stored bit patterns (u32 views of f32, FP16 / E4M3 rows as stored):
there is no tolerance anywhere in this module.  A new slot-option test starts from here, not from a copy of another test file."""
import functools
import inspect

import numpy as np
import pytest

from krasis_amd._lib import KrasisHipError
from tests.test_decode_gpu import build as build_hybrid
from tests.test_mla_gpu import build as build_mla

F = np.float32
U = np.uint32


def bits(x):
    """a contiguous u32 copy of the array's bit patterns"""
    return np.ascontiguousarray(x).view(U).copy()


def pages(n, pt):
    return (n + pt - 1) // pt


def toks(rng, d, n):
    return [int(x) for x in rng.integers(0, d["V"], n)]


def _reference(K, st, d, prompt, first, n_steps):
    K.start(st, d, prompt)
    out, tok, pos = [], first, len(prompt)
    for _ in range(n_steps):
        st.decode_step(tok, pos)
        out.append((st.read_logits().view(U).copy(), st.last_token()))
        tok = out[-1][1]; pos += 1
    return out, K.snap(st, d, pos)


class Gqa:
    """the hybrid linear-attention + GQA test model and its single-sequence reference helpers"""
    @staticmethod
    def build(fp8=False, **kw):
        st, eng, orc, keep, d = build_hybrid(**kw)
        if fp8:
            st.set_kv_dtype(True); d["fp8"] = True
        return st, (eng, orc, keep), d

    @staticmethod
    def start(st, d, prompt):
        """the store's own sequence = prompt (zero state, then the prompt pass; decode_step token by token where the prompt pass refuses the geometry, dv < dk)"""
        st.reset_decode_state(d["kv_max"])
        if prompt and d["dv"] >= d["dk"]:
            st.prefill(prompt, 0)
        else:
            for i, t in enumerate(prompt):
                st.decode_step(t, i)

    @staticmethod
    def reference(st, d, prompt, first, n_steps):
        """decode_step alone: per step (logits bits, greedy id); then the state snapshot after the steps"""
        return _reference(Gqa, st, d, prompt, first, n_steps)

    @staticmethod
    def snap(st, d, upto):
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

    @staticmethod
    def same(a, b):
        assert len(a) == len(b)
        for x, y in zip(a, b):
            assert x[0] == y[0] and x[1] == y[1]
            assert np.array_equal(x[2], y[2]), (x[0], x[1], "conv" if x[0] == "la" else "k")
            assert np.array_equal(x[3], y[3]), (x[0], x[1], "recur" if x[0] == "la" else "v")

    @staticmethod
    def upto(snap, n):
        return [(k, li, a[:n], b[:n]) for k, li, a, b in snap]


class Mla:
    """the MLA test model and its single-sequence reference helpers"""
    @staticmethod
    def build(fp8=False, **kw):
        st, eng, orc, keep, d = build_mla(**kw)
        d["fp8"] = fp8
        if fp8:
            st.set_kv_dtype(True)
        return st, (eng, keep), d

    @staticmethod
    def start(st, d, prompt):
        """the store's own sequence = prompt (build leaves random caches: zero state first, then the prompt pass)"""
        st.reset_decode_state(d["kv_max"])
        if prompt:
            st.prefill(prompt, 0)

    @staticmethod
    def reference(st, d, prompt, first, n_steps):
        """decode_step alone: per step (logits bits, greedy id); then the caches after the steps"""
        return _reference(Mla, st, d, prompt, first, n_steps)

    @staticmethod
    def snap(st, d, pos):
        """rows [0, pos) of the latent and the rope-key cache of every layer, as stored (uint16: FP16, uint8: E4M3)"""
        t = np.uint8 if d["fp8"] else np.uint16
        out = []
        for li in range(d["nL"]):
            ck = np.empty((d["kv_max"], d["klr"]), t); kp = np.empty((d["kv_max"], d["rd"]), t)
            st.get_decode_state(li, ck, kp, None, None)
            out.append((ck[:pos].copy(), kp[:pos].copy()))
        return out

    @staticmethod
    def same(got, want):
        assert len(got) == len(want)
        for li, ((ck, kp), (rck, rkp)) in enumerate(zip(got, want)):
            assert np.array_equal(ck, rck), ("latent rows", li)
            assert np.array_equal(kp, rkp), ("rope-key rows", li)

    @staticmethod
    def upto(snap, n):
        return [(a[:n], b[:n]) for a, b in snap]


def state_error(call, *needles):
    """the call is refused with KR_ERR_STATE (RuntimeError, not a HIP failure) and its message names every needle"""
    with pytest.raises(RuntimeError) as e:
        call()
    assert not isinstance(e.value, KrasisHipError), e.value
    for s in needles:
        assert s in str(e.value), (s, str(e.value))


def slot_state(K, st, d, slot, upto):
    """the slot's sequence loaded into the zeroed store -> its snapshot"""
    st.reset_decode_state(d["kv_max"])
    st.load_slot(slot, upto)
    return K.snap(st, d, upto)


def fill_prefix(st, d, prefix, slots):
    """the prefix, by the exact prompt pass on the store's own sequence, into every slot of `slots`"""
    st.reset_decode_state(d["kv_max"])
    if prefix:
        st.prefill(prefix, 0)
    for s in slots:
        st.save_slot(s, len(prefix))


def fill_upto(st, d, seq, want):
    """want = [(slot, n)]: the first n tokens of seq, by the exact prompt pass on the store's own sequence, into the slot (one pass serves every n)"""
    st.reset_decode_state(d["kv_max"])
    top = max(n for _, n in want)
    if top:
        st.prefill(list(seq[:top]), 0)
    for s, n in want:
        st.save_slot(s, n)


def equal(K, a, b, where=""):
    """two results (ids, logits, slot states) of one scenario: bit for bit"""
    assert [int(x) for x in a[0]] == [int(x) for x in b[0]], ("ids", where)
    assert np.array_equal(bits(a[1]), bits(b[1])), ("logits", where)
    assert len(a[2]) == len(b[2])
    for x, y in zip(a[2], b[2]):
        K.same(x, y)


def off_on(st, opt, scenario, **other):
    """scenario(st) -> (ids, logits, states) on slots it creates and fills itself, once with the option off and once with it on; `other` options stay set for both"""
    out = []
    for on in (0, 1):
        for o, v in other.items():
            st.set_option(o, v)
        st.set_option(opt, on)
        out.append(scenario(st))
        st.set_option(opt, 0)
        for o in other:
            st.set_option(o, 0)
    return out


def options_reset(stores, settings, prefill_chunk=False):
    """-> the autouse fixture a module binds to a name of its own.  After each test every store of `stores` (a list, or a callable that gives one) gets, in
    order, each setting (a name: off; a (name, value) pair: that value), the exact attention mode, and with `prefill_chunk` the default prompt chunk"""
    @pytest.fixture(autouse=True)
    def fixture():
        yield
        for st in (stores() if callable(stores) else stores):
            for o in settings:
                st.set_option(*((o, 0) if isinstance(o, str) else o))
            st.set_attention_mode(False)
            if prefill_chunk:
                st.set_prefill_chunk(0)
    return fixture


def cached(f):
    """lru_cache on the bound arguments, defaults applied: f(a, b), f(a, b, kv_max=<the default>) and f(a, b, <the default>) are one entry"""
    sig = inspect.signature(f)
    hit = functools.lru_cache(maxsize=None)(f)

    @functools.wraps(f)
    def call(*a, **kw):
        b = sig.bind(*a, **kw)
        b.apply_defaults()
        return hit(*b.args, **b.kwargs)
    return call


def store_cache(stores, minimum=None):
    """-> the decorator of a module's "one store per geometry" function: build(...) -> (st, keep, d) runs once per geometry (cached); the store gets option
    `minimum` = 1 where one is named and joins the module's `stores`"""
    def wrap(build):
        @functools.wraps(build)
        def built(*a):
            out = build(*a)
            if minimum:
                out[0].set_option(minimum, 1)
            stores.append(out[0])
            return out
        return cached(built)      # functools.wraps: the cache binds the call against build's own signature
    return wrap
