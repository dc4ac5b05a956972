"""What a caller sees when the opt-in forms of the batched pass over device slots are refused, alone and together (docs/design/39-slot-option-rules.md).
The eleven options have one ordered list of refusals; which of two refusing options speaks first is part of the contract, and it is held here where it can
be seen: through set_option, set_attention_mode, create_slots and step_multi only.  Every case is one step_multi of slot 0, token 1, position 0 under a set
of options; its outcome -- "ok", or the exception's type and whole message -- is compared with tests/golden/slot_option_refusals.json, which was recorded by
record() below on the commit before the refusals became one table, and is never made from the code under test.

Stores: the test builders at their smallest sizes, slots of 32 positions, flat and paged.  Main stores (linear attention only, GQA only, MLA only, the
hybrid) take no option, each option alone, every pair, all eleven, and each option alone under the attention-mode bit; the outlier stores (three heads per
KV head, three MLA heads, dk = dv = 64) take the options alone.  The coverage conditions at the end are computed from the fixture, so a thin one fails."""
import itertools
import re

import pytest

from tests.util import FLAGS as ALL_FLAGS, refusal_case as key, slot_option_refusals

pytestmark = pytest.mark.gpu
MAX_SEQ, PT = 32, 32
RULES = ALL_FLAGS[2:]      # the nine options of the rule list, in its order; the two GQA flash-decode options have a clause of their own ahead of it
LAYOUTS = ("flat", "paged")


def _gqa(**kw):
    from tests.test_multi_paged_gpu import Gqa
    return Gqa.build(kv_max=MAX_SEQ + 8, **kw)


def _mla(**kw):
    from tests.test_multi_paged_gpu import Mla
    return Mla.build(kv_max=MAX_SEQ + 8, **kw)


STORES = {      # name -> (builder, main store)
    "la": (lambda: _gqa(kinds=["la", "la"]), True),
    "gqa": (lambda: _gqa(kinds=["gqa", "gqa"]), True),
    "mla": (lambda: _mla(), True),
    "hybrid": (lambda: _gqa(), True),
    "gqa-3-per-kv": (lambda: _gqa(kinds=["gqa", "gqa"], nh=6), False),
    "mla-3-heads": (lambda: _mla(klr=256, nh=3, seed=4), False),
    "hybrid-dk64": (lambda: _gqa(la_dkdv=(64, 64)), False),
}


def cases(main):
    """(flags, attention-mode bit) of every case of a store, in the fixture's order"""
    singles = [((f,), False) for f in ALL_FLAGS]
    if not main:
        return singles
    return [((), False)] + singles + [(p, False) for p in itertools.combinations(ALL_FLAGS, 2)] + [(ALL_FLAGS, False)] + [((f,), True) for f in ALL_FLAGS]


def observe(st, flags, mode):
    """one step under the options, which are cleared again whatever happens"""
    try:
        for f in flags:
            st.set_option(f, 1)
        st.set_attention_mode(mode)
        try:
            st.step_multi([0], [1], [0])
        except Exception as e:
            return "%s: %s" % (type(e).__name__, e)
        return "ok"
    finally:
        st.set_attention_mode(False)
        for f in flags:
            st.set_option(f, 0)


def _slots(st, layout):
    st.create_slots(2, MAX_SEQ, **(dict(page_tokens=PT, n_pages=2) if layout == "paged" else {}))


def run_store(name, layout):
    """every case's outcome; then, options cleared, slot 1 (which no case touched) steps to the image an untouched step gives"""
    build, main = STORES[name]
    st, keep, d = build()
    _slots(st, layout)
    want_id = st.step_multi([1], [1], [0])
    want = st.export_slot(1, 1).tobytes()
    _slots(st, layout)
    got = {key(f, m): observe(st, f, m) for f, m in cases(main)}
    assert st.step_multi([1], [1], [0]) == want_id
    assert st.export_slot(1, 1).tobytes() == want, "the slot after a step differs from an untouched step's"
    return got


def record():
    """the fixture: a table of the distinct outcomes and one index per case (run on the commit before the rule table, from a job script)"""
    msgs, out = ["ok"], {}
    for name in STORES:
        for layout in LAYOUTS:
            got = run_store(name, layout)
            for m in got.values():
                if m not in msgs:
                    msgs.append(m)
            out["%s/%s" % (name, layout)] = {k: msgs.index(m) for k, m in got.items()}
    return {"messages": msgs, "stores": out}


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("name", list(STORES))
def test_every_case_gives_the_recorded_outcome(name, layout):
    fx = slot_option_refusals()
    want = {k: fx["messages"][i] for k, i in fx["stores"]["%s/%s" % (name, layout)].items()}
    assert sorted(want) == sorted(key(f, m) for f, m in cases(STORES[name][1])), "the fixture holds other cases than the enumeration"
    got = run_store(name, layout)
    bad = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert not bad, bad


# ---- the fixture's own coverage ------------------------------------------------------------------------------------------------------------------------------
def _table():
    fx = slot_option_refusals()
    return {s: {k: fx["messages"][i] for k, i in c.items()} for s, c in fx["stores"].items()}


def _own(msg, opt):
    """the refusal is this option's own: its words name the option and no other of the eleven"""
    named = set(re.findall(r"multi_[a-z_]+", msg)) & set(ALL_FLAGS)
    return msg != "ok" and opt in named and (named == {opt} or "options both claim" in msg)


def test_fixture_orders_every_pair_of_the_rule_list():
    """for every pair of the nine, some store refuses each alone in its own words, and the pair's outcome is one of the two: the fixture says who speaks first"""
    table = _table()
    for a, b in itertools.combinations(RULES, 2):
        shown = [s for s, c in table.items() if key((a, b), False) in c and _own(c[key((a,), False)], a) and _own(c[key((b,), False)], b)
                 and c[key((a,), False)] != c[key((b,), False)] and c[key((a, b), False)] in (c[key((a,), False)], c[key((b,), False)])]
        assert shown, (a, b)


# every message of the rule table that a case can reach, as the words around its numbers.  Not reached here: the LDS-window failures; "multi_mla_fast"'s
# geometry rule (more than 64 heads: tests/test_multi_mla_fast_gpu.py builds that store); "multi_extend_la_chunk"'s "layer is MLA" (no builder gives a store
# with linear-attention and MLA layers); "multi_extend_la_exact"'s geometry rule (it needs dk > dv, which none of the outlier stores has)
WORDS = [
    'the "multi_mla_fast" option covers MLA layers only: this store has none (set the option to 0 for the exact step)',
    'the "multi_extend_mla_flash" option covers MLA layers only: this store has none (set the option to 0 for the exact pass)',
    'the "multi_extend_flash" option covers GQA layers only: layer 0 is MLA (set the option to 0 for the exact pass)',
    'the "multi_extend_flash" option covers GQA layers only: this store has none (set the option to 0 for the exact pass)',
    "multi_extend_flash: GQA geometry nh 6 nkv 2 head_dim 64 not covered (heads per KV head must divide 128, head_dim 64 / 128 / 256)",
    'the "multi_extend_la_chunk" option covers linear-attention layers only: this store has none (set the option to 0 for the exact pass)',
    "multi_extend_la_chunk: linear-attention geometry nk 2 nv 4 dk 64 dv 64 not covered (dk = dv = 128, whole value-head groups per key head)",
    'the "multi_extend_exact_mfma" and "multi_extend_flash" options both claim the runs of >= 2 tokens of the GQA layers: set one of them to 0',
    'the "multi_extend_exact_mfma" option covers GQA layers only: this store has none (set the option to 0)',
    "multi_extend_exact_mfma: GQA geometry nh 6 nkv 2 head_dim 64 not covered (heads per KV head must divide 32, head_dim 64 / 128 / 256; set the option to 0 for the per-row kernel)",
    'the "multi_extend_mla_exact_mfma" and "multi_extend_mla_flash" options both claim the runs of >= 2 tokens of the MLA layers: set one of them to 0',
    'the "multi_extend_mla_exact_mfma" option covers MLA layers only: this store has none (set the option to 0)',
    "multi_extend_mla_exact_mfma: MLA geometry heads 3 kv_lora_rank 256 rope 64 not covered (the head count must divide 32, kv_lora_rank 512 / 256, rope 64; set the option to 0 for the per-row kernel)",
    'the "multi_attn_exact_split" option covers GQA layers only: this store has none (set the option to 0)',
    'the "multi_mla_exact_split" option covers MLA layers only: this store has none (set the option to 0)',
    'the "multi_extend_la_exact" and "multi_extend_la_chunk" options both claim the long runs of the linear-attention layers: set one of them to 0',
    'the "multi_extend_la_exact" option covers linear-attention layers only: this store has none (set the option to 0)',
    # ahead of the list: the GQA flash-decode options' MLA clause, the attention-mode bit, the entry point's paged refusal
    'the "multi_attn_fast" option covers GQA layers only: layer 0 is MLA (set the option to 0 for the exact step)',
    'the "multi_attn_fast_paged" option covers GQA layers only: layer 0 is MLA (set the option to 0 for the exact step)',
    "the multi-sequence step is exact-mode only: the attention mode has tolerance bits set (1)",
    '"multi_attn_fast" does not read paged slots (kr_decode_slots_create_paged): set "multi_attn_fast_paged", clear the option or create flat slots',
]


def test_fixture_produces_every_reachable_message():
    fx = slot_option_refusals()
    types = {"RuntimeError: ", "ValueError: "}
    texts = {m.split(": ", 1)[1] for m in fx["messages"] if m != "ok"}
    assert all(m == "ok" or m[:m.index(": ") + 2] in types for m in fx["messages"]), "a case ended in a HIP failure"
    missing = [w for w in WORDS if w not in texts]
    assert not missing, missing


def test_fixture_catches_the_known_traps():
    t = _table()
    one = lambda store, *flags: t[store][key(flags, False)]
    # an MLA-only store: "multi_extend_flash" asks "a layer is MLA" first, "multi_extend_la_chunk" asks "has none" first
    assert "layer 0 is MLA" in one("mla/flat", "multi_extend_flash") and "this store has none" in one("mla/flat", "multi_extend_la_chunk")
    # paged slots under "multi_attn_fast" alone: every rule but "multi_mla_fast" stands back and the entry point's paged refusal speaks
    for f in RULES[1:]:
        for store in ("la/paged", "gqa/paged", "hybrid/paged"):
            assert one(store, "multi_attn_fast", f).startswith('RuntimeError: "multi_attn_fast" does not read paged slots'), (store, f)
        assert _own(one("gqa/paged", "multi_attn_fast_paged", f), f) or one("gqa/paged", "multi_attn_fast_paged", f) == "ok", f      # with the paged option nobody stands back
    assert _own(one("gqa/paged", "multi_attn_fast", "multi_mla_fast"), "multi_mla_fast")
    # "multi_extend_la_exact" is asked behind "multi_mla_exact_split", although it came to the chain later
    assert _own(one("gqa/flat", "multi_mla_exact_split", "multi_extend_la_exact"), "multi_mla_exact_split")
    # a rival is named before "has none", and only once the rival's own clause has passed
    assert "both claim" in one("gqa/flat", "multi_extend_flash", "multi_extend_exact_mfma")
    assert _own(one("la/flat", "multi_extend_flash", "multi_extend_exact_mfma"), "multi_extend_flash")
