"""The exact batched multi-sequence step with and without "multi_mla_exact_split" (docs/design/31-multi-mla-exact-split.md) on the 27-layer DeepSeek-V2-Lite
synthetic (bench.build_v2lite, E4M3 latent caches, the model of multi_mla_throughput.py), on flat slots and, with --page-tokens N, on paged slots of N positions
per page as well.

Every slot holds the fill_state_synthetic state saved at position P.  Per (P, B) the variants alternate inside this one process -- flat option off, flat option
on, paged off, paged on -- and the whole table is measured --rounds times (default 3): per variant the median wall time of 12 step_multi calls after 3 of warm-up
(a call returns after the ids' read-back), every variant stepping the same rows from the same position.  "multi_mla_exact_split_min" is 1 throughout, so the
option-on leg takes the split at every P.  Behind the table: verify_multi of 1 + 4 tokens at B = 16, P = 4096, off / on, measured the same way (each pass
committed as nothing, so every pass verifies the same rows).  Then, per cell, the median over the rounds and the spread (max - min over the rounds).
--off-only: only the option-off legs and no option is named: how a library without the option (KRASIS_HIP_LIB = the parent commit's build) is measured beside
this one, to show that the option-off step did not move.
--profile: only B = 64 steps at P = 4096 with the option on (paged with --page-tokens), for a rocprofv3 --kernel-trace --stats run of its own.

    python tools/probes/multi_mla_exact_split_throughput.py [out.txt] [--page-tokens N] [--rounds R] [--off-only] [--profile]
"""
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

import bench  # noqa: E402

BS = (1, 16, 64, 256)
PS = (512, 1024, 2048, 4096)
WARM, REPS = 3, 12
OPT, MIN = "multi_mla_exact_split", "multi_mla_exact_split_min"
VB, VP, VDRAFT = 16, 4096, 4


def step_ms(st, B, P):
    ts = []
    for i in range(WARM + REPS):
        t0 = time.perf_counter()
        st.step_multi(list(range(B)), [(i * 7 + b) % 1000 for b in range(B)], [P + i] * B)
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts[WARM:]) * 1e3


def verify_ms(st, B, P):
    ts = []
    for i in range(WARM + REPS):
        t0 = time.perf_counter()
        st.verify_multi(list(range(B)), [[(i * 7 + b + t) % 1000 for t in range(1 + VDRAFT)] for b in range(B)], [P] * B)
        ts.append(time.perf_counter() - t0)
        st.commit_multi([0] * B)
    return statistics.median(ts[WARM:]) * 1e3


def flag(argv, name, default):
    return int(argv[argv.index(name) + 1]) if name in argv else default


def main():
    argv = sys.argv[1:]
    page_tokens, rounds = flag(argv, "--page-tokens", 0), flag(argv, "--rounds", 3)
    profile, off_only = "--profile" in argv, "--off-only" in argv
    skip = {i + 1 for i, a in enumerate(argv) if a in ("--page-tokens", "--rounds")}
    args = [a for i, a in enumerate(argv) if not a.startswith("--") and i not in skip]
    out_path = args[0] if args else None
    kv = 4096 + 160
    eng, st, keep = bench.build_v2lite(0, 0, 27, rope_len=kv, kv_fp8=True)
    lines = []

    def log(s):
        print(s, flush=True); lines.append(s)

    def slots(n, P, paged, reach=WARM + REPS):
        """n slots at position P; paged: a pool that holds exactly the rows the calls of one variant reach"""
        if paged:
            st.create_slots(n, kv, page_tokens=page_tokens, n_pages=n * ((P + reach + page_tokens - 1) // page_tokens))
        else:
            st.create_slots(n, kv)
        for s in range(n):
            st.save_slot(s, P)

    st.fill_state_synthetic(kv, seed=99)                      # the store's own sequence: what every slot is saved from; the batched calls leave it alone
    if not off_only:
        st.set_option(MIN, 1)
    if profile:
        slots(64, 4096, page_tokens > 0)
        st.set_option(OPT, 1)
        for i in range(6):
            st.step_multi(list(range(64)), [i] * 64, [4096 + i] * 64)
        return
    kinds = [("flat", False)] + ([(f"paged {page_tokens}", True)] if page_tokens else [])
    legs = (0,) if off_only else (0, 1)
    names = [k + (" on" if on else " off") for k, _ in kinds for on in legs]
    lib = os.environ.get("KRASIS_HIP_LIB", "the library of this tree")
    log(f"library: {lib}; ms per step_multi, median of {REPS} after {WARM}; {rounds} rounds")
    log(f"{'round':>5} {'P':>5} {'B':>4} " + " ".join(f"{n:>13}" for n in names))
    cells = {}
    for r in range(rounds):
        for P in PS:
            for B in BS:
                ms = []
                for _, paged in kinds:
                    for on in legs:
                        slots(B, P, paged)                   # every variant steps the same rows from the same position
                        if not off_only:
                            st.set_option(OPT, on)
                        ms.append(step_ms(st, B, P))
                        if not off_only:
                            st.set_option(OPT, 0)
                cells.setdefault((P, B), []).append(ms)
                log(f"{r:>5} {P:>5} {B:>4} " + " ".join(f"{x:>13.3f}" for x in ms))
    log(f"ms per verify_multi of 1 + {VDRAFT} tokens, B = {VB}, P = {VP}, median of {REPS} after {WARM}")
    log(f"{'round':>5} " + " ".join(f"{n:>13}" for n in names))
    for r in range(rounds):
        ms = []
        for _, paged in kinds:
            for on in legs:
                slots(VB, VP, paged, reach=1 + VDRAFT)
                if not off_only:
                    st.set_option(OPT, on)
                ms.append(verify_ms(st, VB, VP))
                if not off_only:
                    st.set_option(OPT, 0)
        cells.setdefault(("verify", VB), []).append(ms)
        log(f"{r:>5} " + " ".join(f"{x:>13.3f}" for x in ms))
    log("")
    log("median over the rounds (spread = max - min over the rounds, in % of the median)")
    log(f"{'P':>6} {'B':>4} " + " ".join(f"{n:>21}" for n in names))
    for (P, B), rows in cells.items():
        cols = list(zip(*rows))
        log(f"{P:>6} {B:>4} " + " ".join(f"{statistics.median(c):>12.3f} ({(max(c) - min(c)) / statistics.median(c) * 100:>5.2f}%)" for c in cols))
    if out_path:
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
