"""The batched multi-sequence step with and without the MLA split-KV flash-decode option ("multi_mla_fast", docs/design/24-multi-mla-fast.md) on the
27-layer DeepSeek-V2-Lite synthetic (bench.build_v2lite, E4M3 latent caches, the model of multi_mla_throughput.py), on flat slots and on paged slots of
--page-tokens positions per page (default 64).

Every slot holds the fill_state_synthetic state saved at position P (512, 4096).  Per (P, B) the variants alternate inside this one process -- flat option
off, flat option on, paged option off, paged option on -- and the whole table is measured --rounds times (default 3): per variant the median wall time of 12
step_multi calls after 3 of warm-up (a call returns after the ids' read-back), every variant stepping the same rows from the same position.  The summary
gives the median over the rounds and their spread (max - min) per cell, option-on against option-off and paged-on against flat-on.
--profile: only B = 64 steps at P = 4096 with the option on (paged unless --page-tokens 0), for a rocprofv3 --kernel-trace --stats run of its own.

    python tools/probes/multi_mla_fast_throughput.py [out.txt] [--page-tokens N] [--rounds R] [--profile]
"""
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

import bench  # noqa: E402

OPT = "multi_mla_fast"
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
    page_tokens, rounds = flag(argv, "--page-tokens", 64), flag(argv, "--rounds", 3)
    profile = "--profile" in argv
    skip = {i + 1 for i, a in enumerate(argv) if a in ("--page-tokens", "--rounds")}
    args = [a for i, a in enumerate(argv) if not a.startswith("--") and i not in skip]
    out_path = args[0] if args else None
    kv = 4096 + 160
    eng, st, keep = bench.build_v2lite(0, 0, 27, rope_len=kv, kv_fp8=True)
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
        st.set_option(OPT, 1)
        for i in range(6):
            st.step_multi(list(range(64)), [i] * 64, [4096 + i] * 64)
        return
    kinds = [("flat", False)] + ([(f"paged {page_tokens}", True)] if page_tokens else [])
    log(f"ms per step_multi, median of {REPS} after {WARM}; {rounds} rounds")
    log(f"{'round':>5} {'P':>5} {'B':>4} " + " ".join(f"{k + ' off':>13} {k + ' on':>13}" for k, _ in kinds))
    cells = {}
    for r in range(rounds):
        for P in PS:
            for B in BS:
                ms = []
                for _, paged in kinds:
                    for on in (0, 1):
                        slots(B, P, paged)                   # every variant steps the same rows from the same position
                        st.set_option(OPT, on)
                        ms.append(step_ms(st, B, P))
                        st.set_option(OPT, 0)
                cells.setdefault((P, B), []).append(ms)
                log(f"{r:>5} {P:>5} {B:>4} " + " ".join(f"{x:>13.3f}" for x in ms))
    log("")
    log("median over the rounds (spread = max - min over the rounds)")
    log(f"{'P':>5} {'B':>4} " + " ".join(f"{k + ' off':>20} {k + ' on':>20}" for k, _ in kinds) + f" {'off / on (flat)':>16}" + (f" {'paged on / flat on':>19}" if page_tokens else ""))
    for (P, B), rows in cells.items():
        cols = list(zip(*rows))
        med = [statistics.median(c) for c in cols]
        txt = " ".join(f"{m:>11.3f} (+-{max(c) - min(c):.3f})".rjust(20) for m, c in zip(med, cols))
        log(f"{P:>5} {B:>4} {txt} {med[0] / med[1]:>16.2f}" + (f" {med[3] / med[1]:>19.3f}" if page_tokens else ""))
    if out_path:
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
