""""multi_attn_fast_paged" = 2 (docs/design/44-multi-attn-fast-share.md): rows of a batched pass that read the same cache rows for a full chunk share a workgroup
of the split-KV chunk pass.  Every scenario runs the same calls on slots of 1100 positions (chunks of 128) under value 2 and under value 1 and compares ids,
logits, n_match and the slots' stored rows as bit patterns; a sharing scenario also asks that multi_path_counts()["fd_shared"] grew under 2 and not under 1.
The test model has two KV heads, so G = nh / 2: nh 16 -> G 8 (groups of 4), nh 2 -> G 1 (the cap of 8), nh 6 -> G 3 (32 % 3 != 0), nh 64 -> G 32 (no group)."""
import numpy as np
import pytest

from tests.slots import Gqa, bits, cached, equal, fill_prefix, options_reset, pages, slot_state, toks

pytestmark = pytest.mark.gpu
OPT = "multi_attn_fast_paged"
SLOT_SEQ, PREFIX = 1100, 300      # above gqa_split_min = 1024; two full chunks and a partial one
_stores = []
options_off_afterwards = options_reset(_stores, (OPT, "multi_extend_exact_mfma"))


@cached
def _model(hd, nh, fp8):
    st, keep, d = Gqa.build(fp8, seed=5, hd=hd, nh=nh, kv_max=PREFIX + 20)      # the longest slot is read back at 312 positions
    _stores.append(st)
    rng = np.random.default_rng(hd + nh)
    return st, keep, d, toks(rng, d, PREFIX), toks(rng, d, 200)


def _both(st, scenario, shares, values=(1, 2)):
    """scenario(st, value) -> (ids, logits, states), the option set by the scenario once its slots are filled -> the results, the counter checked"""
    out = []
    for v in values:
        st.multi_path_counts(reset=True)
        out.append(scenario(st, v))
        st.set_option(OPT, 0)
        assert (st.multi_path_counts()["fd_shared"] > 0) == (shares and v == 2), v
    return out


def _forked(st, d, prefix, other, v, pt, private=False, run=False, fork=True):
    """src 0 forked to 5 dsts; with `private` dst 5 is trimmed to 140 and fed other tokens up to the common length (the exact pass), so its second chunk lives in
    pages of its own with other contents.  Then, under value v: every slot takes 0 .. 3 tokens, a step of all six in scrambled order, and one more; with
    `run` the first of them is an extend_multi in which slot 3 brings a run of 9 tokens ("multi_extend_exact_mfma": its row leaves the per-row kernels);
    without `fork` every slot is saved on its own: pages of its own each, though the contents agree"""
    st.create_slots(6, SLOT_SEQ, page_tokens=pt, n_pages=(1 if fork and not private else 6) * pages(PREFIX, pt) + 5 * 2 + 1)
    fill_prefix(st, d, prefix, [0] if fork else range(6))
    if fork:
        st.fork_slot(0, [1, 2, 3, 4, 5], PREFIX)
    if private:
        st.trim_slot(5, 140)
        st.extend_multi([5], [other[:PREFIX - 140]], [140])
    st.set_option(OPT, v)
    slots, taken = [4, 0, 5, 2, 1, 3], {0: 2, 1: 0, 2: 3, 3: 1, 4: 0, 5: 1} if fork else {s: s % 2 for s in range(6)}      # two token rows of one slot would share
    fed = [s for s in slots if taken[s]]
    st.extend_multi(fed, [other[10 * s:10 * s + taken[s]] for s in fed], [PREFIX] * len(fed))
    pos = {s: PREFIX + taken[s] for s in slots}
    ids, lgs = [], []
    for k in range(2):
        if run and k == 0:
            st.set_option("multi_extend_exact_mfma", 1)
            i, lg = st.extend_multi(slots, [other[100:109] if s == 3 else [other[60 + s]] for s in slots], [pos[s] for s in slots], logits=True)
            st.set_option("multi_extend_exact_mfma", 0)
            pos[3] += 8
        else:
            i, lg = st.step_multi(slots, [other[60 + 7 * k + s] for s in slots], [pos[s] for s in slots], logits=True)
        ids += list(i); lgs.append(bits(lg))
        pos = {s: p + 1 for s, p in pos.items()}
    st.set_option(OPT, 0)
    return ids, np.concatenate(lgs), [slot_state(Gqa, st, d, s, pos[s]) for s in slots]


def _verify(st, d, prefix, other, v, paged):
    slots, pos = [2, 0, 1], [280, 279, 281]
    st.create_slots(3, SLOT_SEQ, **(dict(page_tokens=32, n_pages=3 * pages(290, 32)) if paged else {}))
    for s, p in zip(slots, pos):
        fill_prefix(st, d, prefix[:p], [s])
    st.set_option(OPT, v)
    greedy, nm = st.verify_multi(slots, [other[5 * i:5 * i + 5] for i in range(3)], pos)
    keep = [min(int(m), i) + 1 for i, m in enumerate(nm)]
    st.commit_multi(keep)
    pos = [p + k for p, k in zip(pos, keep)]
    ids, lg = st.step_multi(slots, other[20:23], pos, logits=True)
    st.set_option(OPT, 0)
    return [x for g in greedy for x in g] + list(nm) + list(ids), lg, [slot_state(Gqa, st, d, s, p + 1) for s, p in zip(slots, pos)]


QCN = (128, 16, True)      # G = 8, E4M3: the shape the option is for
CASES = {      # name: (model, scenario, whether a group exists).  hd 64 / 128 / 256, FP16 / E4M3 and G 8 / 1 / 3 once each; pages of 32: a tile spans two pages
    "forked pt32": (QCN, lambda *a: _forked(*a, 32), True), "forked pt64": (QCN, lambda *a: _forked(*a, 64), True),
    "forked G1 hd256": ((256, 2, False), lambda *a: _forked(*a, 32), True), "forked G3 hd64": ((64, 6, False), lambda *a: _forked(*a, 64), True),
    # grouping by position instead of by page id would give dst 5 the source's second chunk
    "private pt32": (QCN, lambda *a: _forked(*a, 32, private=True), True), "private pt64": (QCN, lambda *a: _forked(*a, 64, private=True), True),
    # verify_multi of 1 + 4 tokens: the five rows of a slot share its two full chunks, flat or paged; commit and a step follow
    "verify flat": (QCN, lambda *a: _verify(*a, False), True), "verify paged": (QCN, lambda *a: _verify(*a, True), True),
    "beside a run": (QCN, lambda *a: _forked(*a, 64, run=True), True),
    # 32 heads per KV head fill the columns alone; slots that share no page have nothing to share: the pass of value 1, and the counter rests
    "G32": ((64, 64, False), lambda *a: _forked(*a, 64), False), "unrelated": (QCN, lambda *a: _forked(*a, 32, fork=False), False),
}


@pytest.mark.parametrize("case", list(CASES))
def test_value_2_gives_the_bits_of_value_1(case):
    model, scenario, shares = CASES[case]
    st, _, d, prefix, other = _model(*model)
    one, two = _both(st, lambda st, v: scenario(st, d, prefix, other, v), shares)
    equal(Gqa, one, two)


def test_within_stated_tolerance_of_the_exact_paged_step():
    """STATED TOLERANCE (02-numerics.md section 2b): max |on - off| <= 1e-3 max |off| on every row's logits, against the exact paged step (option 0)"""
    st, _, d, prefix, other = _model(128, 16, True)
    off, on = _both(st, lambda st, v: _forked(st, d, prefix, other, v, 64), True, values=(0, 2))
    a, b = off[1].view(np.float32), on[1].view(np.float32)
    ratio = max(float(np.abs(x - y).max() / np.abs(x).max()) for x, y in zip(a, b))
    print(f"largest max|on - off| / max|off| over {len(a)} rows: {ratio:.3e} (bound 1e-3)")
    assert ratio <= 1e-3 and not np.array_equal(off[1], on[1])      # and the flash-decode did run
