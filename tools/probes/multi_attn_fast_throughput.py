"""The batched multi-sequence step with and without the split-KV flash-decode options on the 48-layer QCN synthetic (bench.build_qcn, E4M3 KV, the model
of multi_seq_throughput.py), on flat slots ("multi_attn_fast", docs/design/16-multi-attn-fast.md) and, with --page-tokens N, on paged slots of N positions
per page as well ("multi_attn_fast_paged", docs/design/23-multi-attn-fast-paged.md).

Every slot holds the fill_state_synthetic state saved at position P (512, 4096).  Per (P, B) the variants alternate inside this one process -- flat option
off, flat option on, paged option off, paged option on -- and the whole table is measured --rounds times (default 3): per variant the median wall time of 12
step_multi calls after 3 of warm-up (a call returns after the ids' read-back), every variant stepping the same rows from the same position.  Without
--page-tokens only the two flat variants run, which is also how a library without the paged option (KRASIS_HIP_LIB) is measured beside this one.
--profile: only B = 64 steps at P = 4096 with the option on (paged with --page-tokens), for a rocprofv3 --kernel-trace --stats run of its own.

    python tools/probes/multi_attn_fast_throughput.py [out.txt] [--page-tokens N] [--rounds R] [--profile]
"""
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

import bench  # noqa: E402

BS = (1, 64, 256)
PS = (512, 4096)
WARM, REPS = 3, 12


def step_ms(st, B, P):
    ts = []
    for i in range(WARM + REPS):
        t0 = time.perf_counter()
        st.step_multi(list(range(B)), [(i * 7 + b) % 1000 for b in range(B)], [P + i] * B)
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts[WARM:]) * 1e3


def flag(argv, name, default):
    return int(argv[argv.index(name) + 1]) if name in argv else default


def main():
    argv = sys.argv[1:]
    page_tokens, rounds = flag(argv, "--page-tokens", 0), flag(argv, "--rounds", 3)
    profile = "--profile" in argv
    skip = {i + 1 for i, a in enumerate(argv) if a in ("--page-tokens", "--rounds")}
    args = [a for i, a in enumerate(argv) if not a.startswith("--") and i not in skip]
    out_path = args[0] if args else None
    kv = 4096 + 160
    eng, st, keep = bench.build_qcn(0, 0, 48, rope_len=kv, kv_fp8=True)
    lines = []

    def log(s):
        print(s, flush=True); lines.append(s)

    def slots(n, P, paged):
        """n slots at position P; paged: a pool that holds exactly the rows the steps of one variant reach"""
        if paged:
            st.create_slots(n, kv, page_tokens=page_tokens, n_pages=n * ((P + WARM + REPS + page_tokens - 1) // page_tokens))
        else:
            st.create_slots(n, kv)
        for s in range(n):
            st.save_slot(s, P)

    st.fill_state_synthetic(kv, seed=99)                      # the store's own sequence: what every slot is saved from; the batched calls leave it alone
    if profile:
        slots(64, 4096, page_tokens > 0)
        st.set_option("multi_attn_fast_paged" if page_tokens else "multi_attn_fast", 1)
        for i in range(6):
            st.step_multi(list(range(64)), [i] * 64, [4096 + i] * 64)
        return
    kinds = [("flat", False, "multi_attn_fast")] + ([(f"paged {page_tokens}", True, "multi_attn_fast_paged")] if page_tokens else [])
    lib = os.environ.get("KRASIS_HIP_LIB", "the library of this tree")
    log(f"library: {lib}; ms per step_multi, median of {REPS} after {WARM}; {rounds} rounds")
    log(f"{'round':>5} {'P':>5} {'B':>4} " + " ".join(f"{k + ' off':>13} {k + ' on':>13}" for k, _, _ in kinds))
    for r in range(rounds):
        for P in PS:
            for B in BS:
                ms = []
                for _, paged, opt in kinds:
                    for on in (0, 1):
                        slots(B, P, paged)                   # every variant steps the same rows from the same position
                        st.set_option(opt, on)
                        ms.append(step_ms(st, B, P))
                        st.set_option(opt, 0)
                log(f"{r:>5} {P:>5} {B:>4} " + " ".join(f"{x:>13.3f}" for x in ms))
    if out_path:
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
