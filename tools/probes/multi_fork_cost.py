"""What a slot fork costs and what sharing pages costs the step (kr_decode_slot_fork, docs/design/22-slot-fork.md), on the 48-layer QCN synthetic
(bench.build_qcn, exact mode, E4M3 KV, page_tokens 64).

(a) The wall time of one fork_slot of a 2048-position slot (and of a 2040-position one, whose boundary page is copied) to 1, 8 and 63 destinations,
    against the only way to the same state without it: prefill_slot of the same tokens into each destination.
(b) step_multi at B = 64 and P = 512, 4096 over 64 slots forked from one, against 64 unforked paged slots holding the same state, alternately in one
    process: the median of 12 calls after 3 of warm-up, --rounds R rounds (every median is printed: their spread is the noise).

    python tools/probes/multi_fork_cost.py [out.txt] [--rounds 3]
"""
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

import bench  # noqa: E402

PT, B = 64, 64


def fork_cost(st, kv, log):
    n_prompt = 2048
    tokens = [(i * 31 + 7) % 1000 for i in range(n_prompt)]
    st.create_slots(B, kv, page_tokens=PT, n_pages=B * (n_prompt // PT + 1))
    st.prefill_slot(0, tokens)
    log(f"(a) one slot of {n_prompt} positions to n destinations, ms: fork_slot (median of 5) against prefill_slot into each")
    log(f"{'seq_len':>8} {'n':>3} {'fork':>9} {'prefill':>10} {'ratio':>9}")
    for n in (1, 8, 63):
        dsts = list(range(1, n + 1))
        t0 = time.perf_counter()
        for s in dsts:
            st.prefill_slot(s, tokens)
        t_fill = time.perf_counter() - t0
        for seq_len in (n_prompt, n_prompt - 8):
            ts = []
            for _ in range(6):
                t0 = time.perf_counter(); st.fork_slot(0, dsts, seq_len); ts.append(time.perf_counter() - t0)
            t_fork = statistics.median(ts[1:])
            log(f"{seq_len:>8} {n:>3} {t_fork * 1e3:>9.3f} {t_fill * 1e3:>10.1f} {t_fill / t_fork:>9.0f}")
        pages = st.slot_pages()
        log(f"         pages mapped {sum(pages['per_slot'])}, in use {pages['n_pages'] - pages['free']} of {pages['n_pages']}")


def step_cost(st, kv, rounds, log):
    log(f"(b) step_multi, B = {B}: ms/step (median of 12, per round)")
    slots = list(range(B))
    for P in (512, 4096):
        meds = {"forked": [], "unforked": []}
        for r in range(rounds):
            for kind in ("unforked", "forked"):
                st.create_slots(B, kv, page_tokens=PT, n_pages=B * ((P + 64 + PT - 1) // PT))
                st.fill_state_synthetic(kv, seed=99)
                if kind == "forked":
                    st.save_slot(0, P); st.fork_slot(0, slots[1:], P)
                else:
                    for s in slots:
                        st.save_slot(s, P)
                ts = []
                for i in range(15):
                    t0 = time.perf_counter()
                    st.step_multi(slots, [(i * 7 + b) % 1000 for b in range(B)], [P + i] * B)
                    ts.append(time.perf_counter() - t0)
                meds[kind].append(statistics.median(ts[3:]) * 1e3)
        for kind in ("unforked", "forked"):
            log(f"{P:>5} {kind:>9}   " + "  ".join(f"{m:8.3f}" for m in meds[kind]) + f"   mean {statistics.mean(meds[kind]):8.3f}")


def main():
    rounds = 3
    if "--rounds" in sys.argv:
        i = sys.argv.index("--rounds"); rounds = int(sys.argv[i + 1]); del sys.argv[i:i + 2]
    out_path = sys.argv[1] if len(sys.argv) > 1 else None
    kv = 4096 + 160
    eng, st, keep = bench.build_qcn(0, 0, 48, rope_len=kv, kv_fp8=True)
    lines = []

    def log(s):
        print(s, flush=True); lines.append(s)

    fork_cost(st, kv, log)
    step_cost(st, kv, rounds, log)
    if out_path:
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
