"""Cost of exact speculative greedy decoding on the 48-layer QCN synthetic (bench.build_qcn, exact mode): T(step) of the plain decode step vs
T(n) of kr_decode_verify + kr_decode_commit over n tokens (all drafts right: no rollback; first draft wrong: rollback to 1 token), the projected
rate at per-token acceptance a, and generate_lookup vs generate_batch on a context that repeats the greedy stream.

Timing: wall clock after warm-up, medians.  A verify ends in its one DtoH (the host needs the accepted count before the next pass), so its wall time
is what the loop pays; the step is timed the way the plain loop runs it (step + read of the sampled token), and back to back for reference.
The synthetic model's weights are random: real-text acceptance is not measured here.

    python tools/probes/spec_verify_cost.py [layers=48] [--timing]
"""
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

import bench  # noqa: E402

NS = (1, 2, 3, 5, 9, 16)
ACC = (0.5, 0.7, 0.9)


def main():
    L = int(sys.argv[1]) if len(sys.argv) > 1 and sys.argv[1].isdigit() else 48
    timing = "--timing" in sys.argv
    q = bench.QCN
    eng, st, keep = bench.build_qcn(0, 0, L)
    kv = q["kv_max_seq"]
    reset = lambda: st.fill_state_synthetic(kv, seed=4242)
    pos0, first = 10, 0
    reset()
    for i in range(8):                                   # warm-up: graph capture, scratch, nibble sums
        st.decode_step(first, pos0 + i); st.last_token()
    reset()
    T = st.generate_batch(first, pos0, 160)

    # ---- the plain step
    def step_synced(reps=40):
        reset(); ts = []
        tok = first
        for i in range(reps):
            t0 = time.perf_counter(); st.decode_step(tok, pos0 + i); tok = st.last_token(); ts.append(time.perf_counter() - t0)
        return statistics.median(ts[5:]) * 1e3
    def step_b2b(reps=40):
        reset(); st.last_token()
        t0 = time.perf_counter()
        for i in range(reps):
            st.decode_step(first, pos0 + i)
        st.last_token()
        return (time.perf_counter() - t0) / reps * 1e3
    t_step = step_synced(); t_b2b = step_b2b()

    # ---- verify + commit
    def vc(n, wrong, reps=12):
        ts = []
        for r in range(reps + 2):
            toks = [first] + T[:n - 1]
            if wrong and n > 1:
                toks[1] = (toks[1] + 1) % q["vocab"]
            reset(); st.last_token()
            t0 = time.perf_counter()
            g, m = st.verify(toks, pos0)
            st.commit(m + 1 if not wrong else 1)
            st.last_token()
            ts.append(time.perf_counter() - t0)
            assert (m == n - 1) if not wrong else (m == 0), (n, wrong, m)
        return statistics.median(ts[2:]) * 1e3
    for n in NS:                                           # warm the one-chunk pass at every width once
        vc(n, False, reps=1)
    rows = [(n, vc(n, False), vc(n, True) if n > 1 else None) for n in NS]

    print(f"# QCN synthetic, {L} layers, exact mode, positions {pos0}..; T(step) = {t_step:.3f} ms ({1e3 / t_step:.1f} tok/s) step + token read, "
          f"{t_b2b:.3f} ms back to back")
    print("# n = 1 + k drafts.  T(n) = verify + commit wall time (ends in the verify's DtoH).  E(a) = (1 - a^(k+1)) / (1 - a) tokens per pass at per-token")
    print("# acceptance a; projected rate = E(a) / T(n) (all-right timing; a rejection adds the rollback column's difference)")
    print(f"{'n':>3} {'T(n) ms':>9} {'T/Tstep':>8} {'T(n) rb1':>9} " + " ".join(f"{'E(' + str(a) + ')':>7} {'tok/s':>7}" for a in ACC))
    print(f"{'step':>3} {t_step:9.3f} {1.0:8.2f} {'':>9} " + " ".join(f"{1.0:7.2f} {1e3 / t_step:7.1f}" for a in ACC))
    for n, t_ok, t_rb in rows:
        k = n - 1
        cols = []
        for a in ACC:
            E = (1 - a ** (k + 1)) / (1 - a)
            cols.append(f"{E:7.2f} {E * 1e3 / t_ok:7.1f}")
        print(f"{n:>3} {t_ok:9.3f} {t_ok / t_step:8.2f} {(f'{t_rb:9.3f}' if t_rb else '-'):>9} " + " ".join(cols))

    # ---- the loop on a context that repeats its own greedy stream (acceptance ~1) vs the plain loop
    M = 128
    reset(); st.last_token()
    t0 = time.perf_counter(); ref = st.generate_batch(first, pos0, M); t_plain = time.perf_counter() - t0
    print(f"\n# generate_batch vs generate_lookup, {M} tokens, context = [first] + the greedy stream (drafts right; an upper bound, not real text)")
    print(f"plain generate_batch: {M / t_plain:8.1f} tok/s")
    for md in (3, 4, 8, 15):
        ts = []
        for r in range(3):
            reset(); st.last_token()
            t0 = time.perf_counter(); out = st.generate_lookup(first, pos0, M, context=[first] + T, max_draft=md); ts.append(time.perf_counter() - t0)
            assert out == ref
        s = st.last_lookup_stats
        print(f"generate_lookup max_draft {md:2d}: {M / statistics.median(ts):8.1f} tok/s  ({s['passes']} passes, {s['accepted']} accepted)")
    rng_ctx = [int(x) for x in __import__("numpy").random.default_rng(1).integers(0, q["vocab"], 512)]
    reset(); st.last_token()
    t0 = time.perf_counter(); out = st.generate_lookup(first, pos0, M, context=rng_ctx); t_rand = time.perf_counter() - t0
    assert out == ref
    s = st.last_lookup_stats
    print(f"generate_lookup default, random 512-token context: {M / t_rand:8.1f} tok/s  ({s['passes']} passes, {s['accepted']} accepted)")

    if timing:                                             # where the time of a verify pass goes: host enqueue vs GPU drain (stderr)
        st.set_option("pfm_timing", 1)
        for n in (5, 9):
            reset(); st.last_token()
            g, m = st.verify([first] + T[:n - 1], pos0); st.commit(m + 1)
        st.set_option("pfm_timing", 0)


if __name__ == "__main__":
    main()
