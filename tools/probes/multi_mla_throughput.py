"""Aggregate throughput of the exact multi-sequence decode step (kr_decode_step_multi) over MLA layers on the 27-layer DeepSeek-V2-Lite synthetic
(bench.build_v2lite, exact mode, E4M3 latent caches) against the single-sequence exact step measured in the same run -- all an MLA model could do
before slots covered MLA layers (docs/design/15-multi-mla.md).

Every slot holds the fill_state_synthetic state saved at position P (512, 4096).  Per B: the median wall time of one step_multi after warm-up of
that shape (it returns after the ids' read-back), the aggregate tok/s B / t, and the ratio to the plain step (decode_step + last_token) at the same
positions.  --profile: only B = 64 steps at P = 512 (for a rocprofv3 --kernel-trace --stats run of its own).

    python tools/probes/multi_mla_throughput.py [out.txt] [--profile]
"""
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

import bench  # noqa: E402

BS = (1, 2, 4, 8, 16, 32, 64, 128, 256)
PS = (512, 4096)


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    out_path = args[0] if args else None
    profile = "--profile" in sys.argv
    kv = 4096 + 160
    eng, st, keep = bench.build_v2lite(0, 0, 27, rope_len=kv, kv_fp8=True)
    lines = []

    def log(s):
        print(s, flush=True); lines.append(s)

    nslots = 64 if profile else max(BS)
    log(f"slots: {nslots} x {kv} positions, {st.create_slots(nslots, kv) / 2**30:.1f} GiB")
    for P in ((512,) if profile else PS):
        st.fill_state_synthetic(kv, seed=99)
        for s in range(nslots):
            st.save_slot(s, P)
        if profile:
            for i in range(6):
                st.step_multi(list(range(64)), [i] * 64, [P + i] * 64)
            return
        # the plain exact step (decode_step + read of the sampled token), the way generate_greedy runs it
        tok, ts = 0, []
        for i in range(40):
            t0 = time.perf_counter(); st.decode_step(tok, P + i); tok = st.last_token(); ts.append(time.perf_counter() - t0)
        t1 = statistics.median(ts[8:])
        log(f"P = {P}: single-sequence exact step {t1 * 1e3:.3f} ms = {1 / t1:.1f} tok/s")
        log(f"{'B':>4} {'ms/step':>9} {'tok/s':>9} {'x single':>9}")
        pay = None
        for B in BS:
            reps = 12 if B <= 64 else 8
            ts = []
            for i in range(reps + 3):
                t0 = time.perf_counter()
                st.step_multi(list(range(B)), [(i * 7 + b) % 1000 for b in range(B)], [P + i] * B)
                ts.append(time.perf_counter() - t0)
            t = statistics.median(ts[3:])
            r = B / t * t1
            if pay is None and r > 1.0:
                pay = B
            log(f"{B:>4} {t * 1e3:>9.3f} {B / t:>9.1f} {r:>9.2f}")
        log(f"batching pays from B = {pay}" if pay else "batching does not pay up to B = 256")
    if out_path:
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
