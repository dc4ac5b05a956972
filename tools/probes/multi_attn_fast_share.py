""""multi_attn_fast_paged" = 2 against = 1 (docs/design/44-multi-attn-fast-share.md) on the 48-layer QCN synthetic (bench.build_qcn: 16 query heads over 2 KV
heads, E4M3 KV), pages of 64 positions.

Legs: step_multi of B = 64 / 256 rows whose slots were forked from one prefix of P = 4096 / 512 positions; 64 unrelated rows at 4096 (no group: must equal
value 1 within the spread); verify_multi of 1 + 4 tokens on 16 unrelated slots at 4096, flat and paged (the five rows of a slot share).  Per leg the two values
alternate inside this one process on freshly filled slots, 2 un-timed calls first, then the median and range of 8 timed calls (a call returns after the ids'
read-back); the whole table is measured --rounds times (default 3).

    python tools/probes/multi_attn_fast_share.py [out.txt] [--rounds R]
"""
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

import bench  # noqa: E402

OPT, PT, WARM, REPS = "multi_attn_fast_paged", 64, 2, 8


def timed(call):
    ts = []
    for i in range(WARM + REPS):
        t0 = time.perf_counter()
        call(i)
        ts.append((time.perf_counter() - t0) * 1e3)
    ts = ts[WARM:]
    return statistics.median(ts), min(ts), max(ts)


def main():
    argv = sys.argv[1:]
    rounds = int(argv[argv.index("--rounds") + 1]) if "--rounds" in argv else 3
    out_path = argv[0] if argv and not argv[0].startswith("--") else None
    kv = 4096 + 64
    eng, st, keep = bench.build_qcn(0, 0, 48, rope_len=kv, kv_fp8=True)
    st.fill_state_synthetic(kv, seed=99)
    lines = []

    def log(s):
        print(s, flush=True); lines.append(s)

    def forked(B, P):
        st.create_slots(B, kv, page_tokens=PT, n_pages=P // PT + 2 + B * 2)
        st.save_slot(0, P)
        st.fork_slot(0, list(range(1, B)), P)
        return lambda i: st.step_multi(list(range(B)), [(i * 7 + b) % 1000 for b in range(B)], [P + i] * B)

    def unrelated(B, P):
        st.create_slots(B, kv, page_tokens=PT, n_pages=B * (P // PT + 2))
        for s in range(B):
            st.save_slot(s, P)
        return lambda i: st.step_multi(list(range(B)), [(i * 7 + b) % 1000 for b in range(B)], [P + i] * B)

    def verify(B, P, paged):
        st.create_slots(B, kv, **(dict(page_tokens=PT, n_pages=B * (P // PT + 2)) if paged else {}))
        for s in range(B):
            st.save_slot(s, P)

        def call(i):
            st.verify_multi(list(range(B)), [[(i + b + t) % 1000 for t in range(5)] for b in range(B)], [P] * B)
            st.commit_multi([0] * B)
        return call

    legs = [("forked 64 rows, prefix 4096", lambda: forked(64, 4096)), ("forked 256 rows, prefix 4096", lambda: forked(256, 4096)),
            ("forked 64 rows, prefix 512", lambda: forked(64, 512)), ("forked 256 rows, prefix 512", lambda: forked(256, 512)),
            ("unrelated 64 rows at 4096", lambda: unrelated(64, 4096)),
            ("verify 1+4 on 16 flat slots at 4096", lambda: verify(16, 4096, False)), ("verify 1+4 on 16 paged slots at 4096", lambda: verify(16, 4096, True))]
    log(f"ms per call: median [min, max] of {REPS} after {WARM}; value 1 then value 2 on freshly filled slots; {rounds} rounds")
    for r in range(rounds):
        for name, make in legs:
            got = []
            try:
                for v in (1, 2):
                    call = make()
                    st.set_option(OPT, v)
                    st.multi_path_counts(reset=True)
                    got.append(timed(call) + (st.multi_path_counts()["fd_shared"],))
                    st.set_option(OPT, 0)
            except RuntimeError as e:      # a leg the store refuses is reported, not hidden
                st.set_option(OPT, 0)
                log(f"{r} {name:<38} refused: {e}")
                continue
            log(f"{r} {name:<38} " + "   ".join(f"value {v}: {m:8.3f} [{lo:8.3f}, {hi:8.3f}] shared passes {n:>2}" for v, (m, lo, hi, n) in zip((1, 2), got)))
    if out_path:
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
