"""What a verify + commit over slots costs against the plain batched step (docs/design/18-multi-verify.md), on the 48-layer QCN synthetic
(bench.build_qcn, exact mode, E4M3 KV as bench's plain line).

For B in {16, 64} rows at position 512: step_multi, then verify_multi + commit_multi of runs of 1 + k in {1, 2, 5, 9} tokens whose drafts are the rows'
true greedy continuation (taken from generate_multi first), so every token is accepted and the commit applies all 1 + k.  Median wall time of the
timed repeats after warm-up; verify and commit are also timed apart.  From the ratio T(1 + k) / T(step) the tokens per pass that per-token acceptance
a would give, (1 - a^(k+1)) / (1 - a), and the speed-up over the plain step that follows.

    python tools/probes/multi_verify_cost.py [out.txt]
    python tools/probes/multi_verify_cost.py --step-only      step_multi alone at both B, three rounds (to compare two builds of the library)
    python tools/probes/multi_verify_cost.py --profile        verify + commit passes only (B 64, 1 + k = 5), for a rocprofv3 --kernel-trace --stats run
"""
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

import bench  # noqa: E402

P, BS, RUNS, WARM, REPS = 512, (16, 64), (1, 2, 5, 9), 2, 5
KV = P + 80


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    out_path = args[0] if args else None
    step_only, profile = "--step-only" in sys.argv, "--profile" in sys.argv
    eng, st, keep = bench.build_qcn(0, 0, 48, rope_len=KV, kv_fp8=True)
    lines = []

    def log(s):
        print(s, flush=True); lines.append(s)

    log(f"slots: {max(BS)} x {KV} positions, {st.create_slots(max(BS), KV) / 2**30:.1f} GiB")

    def reset_slots(B):
        st.fill_state_synthetic(KV, seed=99)
        for s in range(B):
            st.save_slot(s, P)

    def t_step(B, n=WARM + REPS):
        reset_slots(B)
        rows, ts = list(range(B)), []
        for i in range(n):
            toks = [(i * 7 + b * 13) % 1000 for b in rows]
            t0 = time.perf_counter(); st.step_multi(rows, toks, [P + i] * B); ts.append(time.perf_counter() - t0)
        return statistics.median(ts[WARM:]), min(ts[WARM:]), max(ts[WARM:])

    if step_only:
        for rnd in range(3):
            for B in BS:
                med, lo, hi = t_step(B, WARM + 10)
                log(f"round {rnd}: step_multi B = {B:>2} at P = {P}: median {med * 1e3:.3f} ms (min {lo * 1e3:.3f}, max {hi * 1e3:.3f})")
        return
    for B in ((64,) if profile else BS):
        rows = list(range(B))
        firsts = [(b * 13 + 5) % 1000 for b in rows]
        n_stream = (WARM + REPS) * max(RUNS)
        reset_slots(B)
        G = st.generate_multi(rows, firsts, [P] * B, n_stream)      # every row's greedy stream: the drafts that are all accepted
        S = [[f] + g for f, g in zip(firsts, G)]
        step = None
        if not profile:
            step = t_step(B)[0]
            log(f"B = {B}: step_multi at P = {P}: {step * 1e3:.2f} ms")
            log(f"{'1 + k':>6} {'verify ms':>10} {'commit ms':>10} {'both ms':>9} {'/ step':>7}   tokens per pass (speed-up over the step) at a = 0.5 / 0.7 / 0.9")
        for c in ((5,) if profile else RUNS):
            reset_slots(B)
            tv, tc = [], []
            for i in range(WARM + REPS):
                runs = [S[b][i * c:(i + 1) * c] for b in rows]
                t0 = time.perf_counter()
                greedy, nm = st.verify_multi(rows, runs, [P + i * c] * B)
                t1 = time.perf_counter()
                st.commit_multi([c] * B)
                t2 = time.perf_counter()
                assert nm == [c - 1] * B, "a draft of the greedy stream was not accepted"
                tv.append(t1 - t0); tc.append(t2 - t1)
            if profile:
                continue
            v, cm = statistics.median(tv[WARM:]), statistics.median(tc[WARM:])
            both = statistics.median([a + b for a, b in zip(tv[WARM:], tc[WARM:])])
            proj = []
            for a in (0.5, 0.7, 0.9):
                tok = (1 - a ** c) / (1 - a)
                proj.append(f"{tok:.2f} ({tok / (both / step):.2f}x)")
            log(f"{c:>6} {v * 1e3:>10.2f} {cm * 1e3:>10.2f} {both * 1e3:>9.2f} {both / step:>7.2f}   " + " / ".join(proj))
    if out_path and not profile:
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
