"""Bit identity of the batched pass over device slots across two builds of the library (docs/design/32-multi-pass-plan.md): the on / off tests bound the
tolerance options, they do not pin their bits.  For each option set: slots are filled by the exact prompt pass, one extend_multi takes a unit row (position 40),
a run of 2 tokens (from position 5) and a run of 70 tokens (from position 17), one step_multi follows on the three slots; printed are sha1[:16] of the logits of
both calls and of every slot's stored state.  The models are the tiny test models: the hybrid ("la", "gqa", "la", "gqa") of tests/test_decode_gpu.build and the
MLA model of tests/test_mla_gpu.build.  Slots hold 1100 positions, so the split-KV options apply; the two *_exact_split_min are 1, so the splits do.

Run it once per library in a process of its own and compare the outputs:

    KRASIS_HIP_LIB=/path/to/other/libkrasis_hip.so python tools/probes/multi_pass_identity.py out_a.txt
    python tools/probes/multi_pass_identity.py out_b.txt
"""
import hashlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

SEQ = 1100
PREFIX, RUNS = (40, 5, 17), (1, 2, 70)
SLOTS = (2, 0, 3)
ALL = ("multi_attn_fast", "multi_attn_fast_paged", "multi_mla_fast", "multi_extend_flash", "multi_extend_mla_flash", "multi_extend_la_chunk", "multi_extend_exact_mfma",
       "multi_extend_mla_exact_mfma", "multi_attn_exact_split", "multi_mla_exact_split")
# (name, options, paged)
HYBRID = [("off", (), False), ("fast", ("multi_attn_fast",), False), ("fast_paged", ("multi_attn_fast_paged",), False), ("pf", ("multi_extend_flash",), False),
          ("lc", ("multi_extend_la_chunk",), False), ("xm", ("multi_extend_exact_mfma",), False), ("xs", ("multi_attn_exact_split",), False),
          ("xm+xs", ("multi_extend_exact_mfma", "multi_attn_exact_split"), False), ("xm+lc", ("multi_extend_exact_mfma", "multi_extend_la_chunk"), False),
          ("fast+pf", ("multi_attn_fast", "multi_extend_flash"), False), ("fast+xm", ("multi_attn_fast", "multi_extend_exact_mfma"), False),
          ("paged off", (), True), ("paged fast_paged", ("multi_attn_fast_paged",), True), ("paged pf+lc", ("multi_extend_flash", "multi_extend_la_chunk"), True),
          ("paged xm+xs", ("multi_extend_exact_mfma", "multi_attn_exact_split"), True)]
MLA = [("off", (), False), ("mla_fast", ("multi_mla_fast",), False), ("mf", ("multi_extend_mla_flash",), False), ("xl", ("multi_extend_mla_exact_mfma",), False),
       ("mla_xs", ("multi_mla_exact_split",), False), ("xl+mla_xs", ("multi_extend_mla_exact_mfma", "multi_mla_exact_split"), False),
       ("mla_fast+mf", ("multi_mla_fast", "multi_extend_mla_flash"), False), ("mla_fast+xl", ("multi_mla_fast", "multi_extend_mla_exact_mfma"), False),
       ("paged off", (), True), ("paged mla_fast+mf", ("multi_mla_fast", "multi_extend_mla_flash"), True), ("paged xl+mla_xs", ("multi_extend_mla_exact_mfma", "multi_mla_exact_split"), True)]


def sha(*arrays):
    h = hashlib.sha1()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()[:16]


def slot_state(st, d, mla, slot, upto):
    """the slot's stored state through the store's own sequence: conv + recurrent state of every linear-attention layer, cache rows [0, upto) of the others"""
    st.reset_decode_state(d["kv_max"])
    st.load_slot(slot, upto)
    out = []
    for li in range(d["nL"]):
        if not mla and d["kinds"][li] == "la":
            cs = np.empty(d["conv_dim"] * 4, np.float32); rs = np.empty(d["nv"] * d["dk"] * d["dv"], np.float32)
            st.get_decode_state(li, None, None, cs, rs); out += [cs, rs]
        else:
            a = np.empty((d["kv_max"], d["klr"] if mla else d["nkv"] * d["hd"]), np.uint16); b = np.empty((d["kv_max"], d["rd"] if mla else d["nkv"] * d["hd"]), np.uint16)
            st.get_decode_state(li, a, b, None, None); out += [a[:upto].copy(), b[:upto].copy()]
    return out


def run(tag, st, d, mla, sets, log):
    rng = np.random.default_rng(11)
    toks = lambda n: [int(x) for x in rng.integers(0, d["V"], n)]
    prefixes, runs = [toks(p) for p in PREFIX], [toks(c) for c in RUNS]
    st.set_option("multi_attn_exact_split_min", 1); st.set_option("multi_mla_exact_split_min", 1)
    for name, options, paged in sets:
        for o in ALL:
            st.set_option(o, 1 if o in options else 0)
        st.create_slots(4, SEQ, **(dict(page_tokens=64, n_pages=3 * ((SEQ + 63) // 64)) if paged else {}))
        for p, s in zip(prefixes, SLOTS):
            st.reset_decode_state(d["kv_max"])
            st.prefill(p, 0)
            st.save_slot(s, len(p))
        ids, lg = st.extend_multi(list(SLOTS), runs, list(PREFIX), logits=True)
        ends = [p + c for p, c in zip(PREFIX, RUNS)]
        ids2, lg2 = st.step_multi(list(SLOTS), [int(i) for i in ids], ends, logits=True)
        for o in ALL:
            st.set_option(o, 0)
        states = [sha(*slot_state(st, d, mla, s, e + 1)) for s, e in zip(SLOTS, ends)]
        log(f"{tag:<7} {name:<20} extend {sha(lg)} step {sha(lg2)} ids {list(map(int, ids))} {list(map(int, ids2))} slots {' '.join(states)}")


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else None
    lines = []

    def log(s):
        print(s, flush=True); lines.append(s)
        if out_path:
            with open(out_path, "w") as f:
                f.write("\n".join(lines) + "\n")

    from tests.test_decode_gpu import build as build_hybrid
    from tests.test_mla_gpu import build as build_mla
    st, eng, orc, keep, d = build_hybrid(seed=3, hd=64, nh=4, kv_max=SEQ, kinds=["la", "gqa", "la", "gqa"])
    d["nL"] = len(d["kinds"])
    run("hybrid", st, d, False, HYBRID, log)
    st2, eng2, orc2, keep2, d2 = build_mla(seed=3, nh=4, kv_max=SEQ)
    run("mla", st2, d2, True, MLA, log)


if __name__ == "__main__":
    main()
