"""Admission cost and mixed prefill + decode passes of the multi-token extend (kr_decode_extend_multi) on the 48-layer QCN synthetic (bench.build_qcn,
exact mode, E4M3 KV as bench's plain line) against the path that was the only one before it -- the store's own prompt pass, then save_slot --
measured in the same run.

Admission: a 512- and a 4096-token prompt into an empty slot.  Before: reset_decode_state + prefill + save_slot (clobbers the store's sequence; the
copy starts with a device synchronise).  Now: prefill_slot (extend_multi over chunks of KR_EXTEND_MAX_TOKENS).  Mixed pass: 63 decode rows at position
512 plus one 256-token prompt chunk.  Before: a 63-row step_multi, then reset + prefill of the 256 tokens + save_slot.  Now: one extend_multi of 64
rows.  Median wall time of the timed repeats after warm-up; every call returns after its ids are back on the host.  --profile: only mixed
extend_multi passes (for a rocprofv3 --kernel-trace --stats run of its own).

    python tools/probes/multi_extend_throughput.py [out.txt] [--profile]
"""
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

import bench  # noqa: E402

P_DECODE, N_DECODE, CHUNK = 512, 63, 256
PROMPTS = (512, 4096)


def timed(fn, warm, reps):
    ts = []
    for i in range(warm + reps):
        t0 = time.perf_counter(); fn(i); ts.append(time.perf_counter() - t0)
    return statistics.median(ts[warm:])


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    out_path = args[0] if args else None
    profile = "--profile" in sys.argv
    kv = 4096 + 160
    eng, st, keep = bench.build_qcn(0, 0, 48, rope_len=kv, kv_fp8=True)
    lines = []

    def log(s):
        print(s, flush=True); lines.append(s)

    nslots = N_DECODE + 2
    log(f"slots: {nslots} x {kv} positions, {st.create_slots(nslots, kv) / 2**30:.1f} GiB")
    toks = lambda n, i=0: [(i * 131 + j * 7) % 1000 for j in range(n)]
    adm, chunk_slot = N_DECODE, N_DECODE + 1

    st.fill_state_synthetic(kv, seed=99)
    for s in range(N_DECODE):
        st.save_slot(s, P_DECODE)
    rows = list(range(N_DECODE))

    def mixed_new(i):
        st.extend_multi(rows + [chunk_slot], [[(i * 7 + b) % 1000] for b in rows] + [toks(CHUNK, i)], [P_DECODE + i] * N_DECODE + [0])

    def mixed_old(i):
        st.step_multi(rows, [(i * 7 + b) % 1000 for b in rows], [P_DECODE + 40 + i] * N_DECODE)
        st.reset_decode_state(kv); st.prefill(toks(CHUNK, i), 0); st.save_slot(chunk_slot, CHUNK)

    if profile:
        for i in range(6):
            mixed_new(i)
        return
    log(f"{'admission':<28} {'tokens':>7} {'before ms':>10} {'now ms':>10} {'now / before':>13}")
    for n in PROMPTS:
        def old(i):
            st.reset_decode_state(kv); st.prefill(toks(n, i), 0); st.save_slot(adm, n)

        def new(i):
            st.prefill_slot(adm, toks(n, i))

        reps = 6 if n <= 512 else 3
        t_old, t_new = timed(old, 2, reps), timed(new, 2, reps)
        log(f"{'prompt -> slot':<28} {n:>7} {t_old * 1e3:>10.2f} {t_new * 1e3:>10.2f} {t_new / t_old:>13.2f}")
    t_step = timed(lambda i: st.step_multi(rows, [(i * 7 + b) % 1000 for b in rows], [P_DECODE + 20 + i] * N_DECODE), 3, 8)
    t_old, t_new = timed(mixed_old, 3, 8), timed(mixed_new, 3, 8)
    log(f"{N_DECODE}-row step_multi alone at P = {P_DECODE}: {t_step * 1e3:.2f} ms")
    log(f"mixed pass, {N_DECODE} decode rows at P = {P_DECODE} + one {CHUNK}-token chunk: before (step_multi, then reset + prefill + save_slot) "
        f"{t_old * 1e3:.2f} ms, now (one extend_multi) {t_new * 1e3:.2f} ms, now / before {t_new / t_old:.2f}")
    log(f"decode rows stand still for: before {(t_old - t_step) * 1e3:.2f} ms per admitted chunk, now {(t_new - t_step) * 1e3:.2f} ms")
    if out_path:
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
