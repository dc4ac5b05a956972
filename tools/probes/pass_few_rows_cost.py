"""Passes of at most 16 token rows with and without "pass_few_rows" (docs/design/34-pass-few-rows.md) on the 48-layer QCN synthetic (bench.build_qcn, E4M3 KV)
or, with --v2lite, on the 27-layer V2-Lite synthetic (bench.build_v2lite, E4M3 KV).

Option off and on alternate inside this one process; per leg the median wall time of 12 calls after 3 of warm-up, the whole table --rounds times (default 3).
Legs: verify + commit of n = 1, 2, 5, 9, 16 tokens on the store's own sequence (drafts = the greedy stream: nothing rolls back); step_multi of B = 1, 2, 4, 8, 16
rows at positions 512 and 4096 with "multi_attn_exact_split" on (minimum 1) in both legs; verify_multi of 1 + 4 tokens on 1 and 3 slots at position 512 (each
pass committed as nothing); and the plain decode step (step + token read) for scale.
--off-only: only the option-off legs and no new option is named: how a library without the option (KRASIS_HIP_LIB = the parent commit's build) is measured
beside this one, to show that the option-off passes did not move.
--group G: "pass_few_rows_group" G for the option-on legs (0 = chosen per launch, the default).
--profile: only verify + commit of n = 5 with the option on, for a rocprofv3 --kernel-trace --stats run of its own.

    python tools/probes/pass_few_rows_cost.py [out.txt] [--v2lite] [--rounds R] [--group G] [--off-only] [--profile]
"""
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

import bench  # noqa: E402

NS = (1, 2, 5, 9, 16)
BS = (1, 2, 4, 8, 16)
PS = (512, 4096)
WARM, REPS = 3, 12
OPT, GROUP = "pass_few_rows", "pass_few_rows_group"
SPLIT, SPLIT_MIN = "multi_attn_exact_split", "multi_attn_exact_split_min"
VDRAFT, VP = 4, 512
POS0, FIRST = 10, 0


def flag(argv, name, default):
    return int(argv[argv.index(name) + 1]) if name in argv else default


def main():
    argv = sys.argv[1:]
    rounds, group = flag(argv, "--rounds", 3), flag(argv, "--group", 0)
    v2lite, off_only, profile = "--v2lite" in argv, "--off-only" in argv, "--profile" in argv
    skip = {i + 1 for i, a in enumerate(argv) if a in ("--rounds", "--group")}
    args = [a for i, a in enumerate(argv) if not a.startswith("--") and i not in skip]
    out_path = args[0] if args else None
    kv = 4096 + 160
    eng, st, keep = bench.build_v2lite(0, 0, 27, rope_len=kv, kv_fp8=True) if v2lite else bench.build_qcn(0, 0, 48, rope_len=kv, kv_fp8=True)
    mla = v2lite
    lines = []

    def log(s):
        print(s, flush=True); lines.append(s)

    reset = lambda: st.fill_state_synthetic(kv, seed=99)

    def arm(on):
        if not off_only:
            st.set_option(OPT, on)
            st.set_option(GROUP, group if on else 0)

    def step_ms():
        reset(); ts, tok = [], FIRST
        for i in range(WARM + 25):
            t0 = time.perf_counter(); st.decode_step(tok, POS0 + i); tok = st.last_token(); ts.append(time.perf_counter() - t0)
        return statistics.median(ts[WARM:]) * 1e3

    def verify_ms(n, T):
        ts = []
        for _ in range(WARM + REPS):
            reset(); st.last_token()
            t0 = time.perf_counter()
            g, m = st.verify([FIRST] + T[:n - 1], POS0)
            st.commit(m + 1); st.last_token()
            ts.append(time.perf_counter() - t0)
            assert m == n - 1, (n, m)
        return statistics.median(ts[WARM:]) * 1e3

    def slots(n, P):
        st.create_slots(n, kv)
        for s in range(n):
            st.save_slot(s, P)

    def step_multi_ms(B, P):
        ts = []
        for i in range(WARM + REPS):
            t0 = time.perf_counter()
            st.step_multi(list(range(B)), [(i * 7 + b) % 1000 for b in range(B)], [P + i] * B)
            ts.append(time.perf_counter() - t0)
        return statistics.median(ts[WARM:]) * 1e3

    def verify_multi_ms(B, P):
        ts = []
        for i in range(WARM + REPS):
            t0 = time.perf_counter()
            st.verify_multi(list(range(B)), [[(i * 7 + b + t) % 1000 for t in range(1 + VDRAFT)] for b in range(B)], [P] * B)
            ts.append(time.perf_counter() - t0)
            st.commit_multi([0] * B)
        return statistics.median(ts[WARM:]) * 1e3

    reset()
    for i in range(8):                                   # warm-up: graph capture, scratch, nibble sums
        st.decode_step(FIRST, POS0 + i); st.last_token()
    reset()
    T = st.generate_batch(FIRST, POS0, 16)
    if profile:
        st.set_option(OPT, 1); st.set_option(GROUP, group)
        for _ in range(6):
            reset(); st.last_token()
            g, m = st.verify([FIRST] + T[:4], POS0); st.commit(m + 1); st.last_token()
        return
    legs = (0,) if off_only else (0, 1)
    names = " ".join(f"{'on' if on else 'off':>9}" for on in legs)
    lib = os.environ.get("KRASIS_HIP_LIB", "the library of this tree")
    log(f"library: {lib}; model: {'V2-Lite synthetic, 27 layers' if v2lite else 'QCN synthetic, 48 layers'}, E4M3 KV; ms, median of {REPS} after {WARM}; {rounds} rounds; "
        f"pass_few_rows_group {group}")
    log(f"decode step + token read: {step_ms():.3f} ms")
    log(f"verify + commit of n tokens at position {POS0} (drafts right)")
    log(f"{'round':>5} {'n':>4} {names}")
    for r in range(rounds):
        for n in NS:
            ms = []
            for on in legs:
                arm(on); ms.append(verify_ms(n, T)); arm(0)
            log(f"{r:>5} {n:>4} " + " ".join(f"{x:>9.3f}" for x in ms))
    log(f"step_multi of B rows at position P, \"{SPLIT}\" on (minimum 1) in every leg")
    log(f"{'round':>5} {'P':>5} {'B':>4} {names}")
    if not mla:
        st.set_option(SPLIT, 1); st.set_option(SPLIT_MIN, 1)
    else:
        st.set_option("multi_mla_exact_split", 1); st.set_option("multi_mla_exact_split_min", 1)
    reset()
    for r in range(rounds):
        for P in PS:
            for B in BS:
                ms = []
                for on in legs:
                    slots(B, P)                          # every leg steps the same rows from the same position
                    arm(on); ms.append(step_multi_ms(B, P)); arm(0)
                log(f"{r:>5} {P:>5} {B:>4} " + " ".join(f"{x:>9.3f}" for x in ms))
    log(f"verify_multi of 1 + {VDRAFT} tokens on B slots at position {VP}")
    log(f"{'round':>5} {'B':>4} {names}")
    for r in range(rounds):
        for B in (1, 3):
            ms = []
            for on in legs:
                slots(B, VP)
                arm(on); ms.append(verify_multi_ms(B, VP)); arm(0)
            log(f"{r:>5} {B:>4} " + " ".join(f"{x:>9.3f}" for x in ms))
    if out_path:
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
