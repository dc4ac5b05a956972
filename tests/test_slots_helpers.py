"""The shared comparisons of tests/slots.py fail when one bit differs: every slot test now relies on these definitions, so they are pinned here on hand-made
snapshots of both kinds, without a GPU (numpy only)."""
import numpy as np
import pytest

from tests.slots import Gqa, Mla, bits, equal, store_cache

U = np.uint32


def _hybrid():
    """one ("la", li, conv, recur) entry and one ("kv", li, k, v) entry"""
    rng = np.random.default_rng(1)
    return [("la", 0, rng.integers(0, 2**32, 24, dtype=U), rng.integers(0, 2**32, 40, dtype=U)),
            ("kv", 1, rng.integers(0, 2**16, (6, 8), dtype=np.uint16), rng.integers(0, 2**16, (6, 8), dtype=np.uint16))]


def _mla():
    """one (latent, rope) layer"""
    rng = np.random.default_rng(2)
    return [(rng.integers(0, 2**16, (6, 16), dtype=np.uint16), rng.integers(0, 2**16, (6, 4), dtype=np.uint16))]


def _copy(snap):
    return [tuple(x.copy() if isinstance(x, np.ndarray) else x for x in layer) for layer in snap]


def _flip(snap, layer, field):
    """a copy in which exactly one element of one array differs by one bit"""
    out = _copy(snap)
    out[layer][field].reshape(-1)[3] ^= 1
    return out


@pytest.mark.parametrize("K,make,places", [(Gqa, _hybrid, [(0, 2), (0, 3), (1, 2), (1, 3)]), (Mla, _mla, [(0, 0), (0, 1)])])
def test_same_passes_on_copies_and_fails_on_one_bit(K, make, places):
    snap = make()
    K.same(_copy(snap), snap)
    for layer, field in places:
        with pytest.raises(AssertionError):
            K.same(_flip(snap, layer, field), snap)
        with pytest.raises(AssertionError):
            K.same(snap, _flip(snap, layer, field))
    with pytest.raises(AssertionError):
        K.same(snap + _copy(snap)[:1], snap)                                # the layer count differs
    with pytest.raises(AssertionError):
        K.same(snap, [])


@pytest.mark.parametrize("K,make", [(Gqa, _hybrid), (Mla, _mla)])
def test_equal_fails_on_one_logits_bit_and_on_one_id(K, make):
    one, next_up = np.array([0x3f800000], U).view(np.float32), np.array([0x3f800001], U).view(np.float32)
    lg = np.stack([one, one])
    res = ([3, 7], lg, [make(), make()])
    equal(K, res, ([3, 7], lg.copy(), [make(), make()]))
    with pytest.raises(AssertionError):
        equal(K, res, ([3, 7], np.stack([one, next_up]), [make(), make()]))
    with pytest.raises(AssertionError):
        equal(K, res, ([3, 8], lg.copy(), [make(), make()]))
    with pytest.raises(AssertionError):
        equal(K, res, ([3, 7], lg.copy(), [make()]))                        # a state is missing
    with pytest.raises(AssertionError):
        equal(K, res, ([3, 7], lg.copy(), [make(), _flip(make(), 0, -1)]))  # one state bit


def test_bits_returns_a_copy():
    x = np.array([1.0, -0.0, 2.5], np.float32)
    b = bits(x)
    assert b.dtype == U and b.tolist() == [0x3f800000, 0x80000000, 0x40200000]
    b[:] = 0
    assert x.tolist() == [1.0, -0.0, 2.5] and np.signbit(x[1])
    assert bits(x[::2]).tolist() == [0x3f800000, 0x40200000]               # a strided view: made contiguous first


def test_upto_slices_what_snap_returns():
    h, m = _hybrid(), _mla()
    got = Gqa.upto(h, 4)
    assert [(g[0], g[1]) for g in got] == [("la", 0), ("kv", 1)]
    assert np.array_equal(got[1][2], h[1][2][:4]) and np.array_equal(got[1][3], h[1][3][:4]) and got[1][2].shape == (4, 8)
    Gqa.same(Gqa.upto(h, 6)[1:], h[1:])
    got = Mla.upto(m, 4)
    assert np.array_equal(got[0][0], m[0][0][:4]) and np.array_equal(got[0][1], m[0][1][:4]) and got[0][1].shape == (4, 4)
    Mla.same(Mla.upto(m, 6), m)


class _Store:
    def __init__(self):
        self.options = []

    def set_option(self, name, value):
        self.options.append((name, value))


def test_store_cache_builds_once_however_the_call_spells_its_defaults():
    stores, calls = [], []

    @store_cache(stores, "some_min")
    def f(a, b, kv_max=600):
        calls.append((a, b, kv_max))
        return _Store(), None, dict(kv_max=kv_max)

    first = f(1, 2)
    assert f(1, 2, kv_max=600) is first and f(1, 2, 600) is first and f(a=1, b=2) is first
    assert calls == [(1, 2, 600)] and stores == [first[0]] and first[0].options == [("some_min", 1)]
    other = f(1, 2, kv_max=1100)
    assert other is not first and f(1, 2, 1100) is other and calls == [(1, 2, 600), (1, 2, 1100)] and stores == [first[0], other[0]]

    plain = []

    @store_cache(plain)
    def g(a):
        return _Store(), None, {}

    assert g(5)[0].options == [] and plain == [g(5)[0]]                     # no minimum named: no option set
