"""What a SAMPLED verify + commit over slots costs against the greedy one, and whether the sampled step kept its speed
(docs/design/19-multi-verify-sample.md), on the 48-layer QCN synthetic (bench.build_qcn, exact mode, E4M3 KV), with the method of multi_verify_cost.py.

Part 1, one process: for B in {16, 64} rows at position 512 and runs of 1 + k in {1, 2, 5, 9} tokens, verify_multi + commit_multi on the rows' greedy
streams against verify_multi_sample + commit_multi on their sampled streams (every slot on the server's default sampler: temperature 0.6, top_k 50,
top_p 0.95), every draft right, so each commit applies all 1 + k tokens.  Median wall time of 5 repeats after 2 warm-ups.

Part 2, --parent-tree DIR (a built checkout of the parent commit): step_multi_sample on this build and on the parent's, alternating, each round a
fresh child process of this file with --step-only --tree.  The margin the step is held to is the parent's own spread between its rounds.

    python tools/probes/multi_verify_sample_cost.py [out.txt] [--parent-tree DIR]
    python tools/probes/multi_verify_sample_cost.py --step-only [--tree DIR]      step_multi_sample alone at both B, on the tree's package and library
"""
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.abspath(__file__)
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(HERE)))


def _opt(name):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else None


sys.path.insert(0, os.path.abspath(_opt("--tree") or ROOT))

import bench  # noqa: E402

P, BS, RUNS, WARM, REPS, ROUNDS = 512, (16, 64), (1, 2, 5, 9), 2, 5, 3
KV = P + 80
SMP = (0.6, 50, 0.95, 0.0)


def step_only(st):
    """median step_multi_sample time per B, one line each (parsed by the parent process)"""
    for B in BS:
        rows, ts = list(range(B)), []
        st.fill_state_synthetic(KV, seed=99)
        for s in rows:
            st.save_slot(s, P)
            st.set_slot_sampler(s, 5, *SMP, 1000 + s)
        for i in range(WARM + 10):
            toks = [(i * 7 + b * 13) % 1000 for b in rows]
            t0 = time.perf_counter(); st.step_multi_sample(rows, toks, [P + i] * B); ts.append(time.perf_counter() - t0)
        print(f"STEP {B} {statistics.median(ts[WARM:]) * 1e3:.4f}", flush=True)


def main():
    skip = {sys.argv.index(o) + 1 for o in ("--tree", "--parent-tree") if o in sys.argv}
    args = [a for i, a in enumerate(sys.argv) if i > 0 and i not in skip and not a.startswith("--")]
    out_path, parent = (args[0] if args else None), _opt("--parent-tree")
    eng, st, keep = bench.build_qcn(0, 0, 48, rope_len=KV, kv_fp8=True)
    st.create_slots(max(BS), KV)
    if "--step-only" in sys.argv:
        return step_only(st)
    lines = []

    def log(s):
        print(s, flush=True); lines.append(s)

    def reset_slots(B, firsts=None):
        st.fill_state_synthetic(KV, seed=99)
        for s in range(B):
            st.save_slot(s, P)
            if firsts:
                st.set_slot_sampler(s, firsts[s], *SMP, 1000 + s)

    log(f"48-layer QCN synthetic, E4M3 KV, P = {P}; sampler of every slot: temperature {SMP[0]}, top_k {SMP[1]}, top_p {SMP[2]}; every draft right; "
        f"median of {REPS} after {WARM} warm-ups")
    for B in BS:
        rows = list(range(B))
        firsts = [(b * 13 + 5) % 1000 for b in rows]
        n_stream = (WARM + REPS) * max(RUNS)
        reset_slots(B)
        G = st.generate_multi(rows, firsts, [P] * B, n_stream)
        reset_slots(B)
        S = st.generate_multi(rows, firsts, [P] * B, n_stream, temperature=SMP[0], top_k=SMP[1], top_p=SMP[2], presence_penalty=SMP[3],
                              rng_seeds=[1000 + s for s in rows])
        streams = {False: [[f] + g for f, g in zip(firsts, G)], True: [[f] + g for f, g in zip(firsts, S)]}
        log(f"B = {B}")
        log(f"{'1 + k':>6} {'rows T':>7} | {'greedy verify':>13} {'commit':>7} {'both ms':>8} | {'sampled verify':>14} {'commit':>7} {'both ms':>8} | {'sampled / greedy':>16}")
        for c in RUNS:
            both = {}
            for sampled in (False, True):
                reset_slots(B, firsts if sampled else None)
                verify = st.verify_multi_sample if sampled else st.verify_multi
                tv, tc = [], []
                for i in range(WARM + REPS):
                    runs = [streams[sampled][b][i * c:(i + 1) * c] for b in rows]
                    t0 = time.perf_counter()
                    ids, nm = verify(rows, runs, [P + i * c] * B)
                    t1 = time.perf_counter()
                    st.commit_multi([c] * B)
                    t2 = time.perf_counter()
                    assert nm == [c - 1] * B, "a draft of the row's own stream was not accepted"
                    tv.append(t1 - t0); tc.append(t2 - t1)
                med = statistics.median
                both[sampled] = (med(tv[WARM:]), med(tc[WARM:]), med([a + b for a, b in zip(tv[WARM:], tc[WARM:])]))
            g, s = both[False], both[True]
            log(f"{c:>6} {B * c:>7} | {g[0] * 1e3:>13.2f} {g[1] * 1e3:>7.2f} {g[2] * 1e3:>8.2f} | {s[0] * 1e3:>14.2f} {s[1] * 1e3:>7.2f} {s[2] * 1e3:>8.2f} | "
                f"{s[2] / g[2]:>16.3f}")
    if parent:
        log(f"step_multi_sample, this build against the parent build, {ROUNDS} rounds alternating (a fresh process each; median of 10 steps after {WARM} warm-ups, ms)")
        got = {"this": {B: [] for B in BS}, "parent": {B: [] for B in BS}}
        for rnd in range(ROUNDS):
            for name, tree in (("this", ROOT), ("parent", os.path.abspath(parent))):
                env = {k: v for k, v in os.environ.items() if k != "KRASIS_HIP_LIB"}
                out = subprocess.run([sys.executable, HERE, "--step-only", "--tree", tree], env=env, capture_output=True, text=True, check=True, timeout=600).stdout
                for ln in out.splitlines():
                    if ln.startswith("STEP "):
                        _, B, ms = ln.split()
                        got[name][int(B)].append(float(ms))
        for B in BS:
            t, p = got["this"][B], got["parent"][B]
            spread = max(p) - min(p)
            verdict = "not slower" if statistics.median(t) <= statistics.median(p) + spread else "SLOWER"
            log(f"B = {B:>2}: this {' '.join(f'{x:.3f}' for x in t)} (median {statistics.median(t):.3f}) | parent {' '.join(f'{x:.3f}' for x in p)} "
                f"(median {statistics.median(p):.3f}, spread {spread:.3f}) -> {verdict} within the parent's spread")
    else:
        log("step_multi_sample against the parent build: not run (no --parent-tree)")
    if out_path:
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
