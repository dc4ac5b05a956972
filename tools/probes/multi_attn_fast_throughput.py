"""The batched multi-sequence step with and without kr_decode_set_option("multi_attn_fast") on the 48-layer QCN synthetic (bench.build_qcn, E4M3 KV,
the model of multi_seq_throughput.py): every point is measured twice in the same run, option off (the exact step: the baseline) then option on
(split-KV flash-decode in the GQA layers, docs/design/16-multi-attn-fast.md).

Every slot holds the fill_state_synthetic state saved at position P (512, 4096).  Per (P, B): the median wall time of one step_multi after
warm-up (it returns after the ids' read-back) for both settings, aggregate tok/s with the option on, and the ratio off / on.
--profile: only B = 64 steps at P = 4096 with the option on (for a rocprofv3 --kernel-trace --stats run of its own).

    python tools/probes/multi_attn_fast_throughput.py [out.txt] [--profile]
"""
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

import bench  # noqa: E402

BS = (1, 8, 64, 256)
PS = (512, 4096)


def step_ms(st, B, P, reps):
    ts = []
    for i in range(reps + 3):
        t0 = time.perf_counter()
        st.step_multi(list(range(B)), [(i * 7 + b) % 1000 for b in range(B)], [P + i] * B)
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts[3:]) * 1e3


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    out_path = args[0] if args else None
    profile = "--profile" in sys.argv
    kv = 4096 + 160
    eng, st, keep = bench.build_qcn(0, 0, 48, rope_len=kv, kv_fp8=True)
    lines = []

    def log(s):
        print(s, flush=True); lines.append(s)

    nslots = 64 if profile else max(BS)
    log(f"slots: {nslots} x {kv} positions, {st.create_slots(nslots, kv) / 2**30:.1f} GiB")
    for P in ((4096,) if profile else PS):
        st.fill_state_synthetic(kv, seed=99)
        for s in range(nslots):
            st.save_slot(s, P)
        if profile:
            st.set_option("multi_attn_fast", 1)
            for i in range(6):
                st.step_multi(list(range(64)), [i] * 64, [P + i] * 64)
            return
        log(f"P = {P}")
        log(f"{'B':>4} {'off ms/step':>12} {'on ms/step':>11} {'on tok/s':>9} {'off / on':>9}")
        for B in BS:
            reps = 10 if B <= 64 else 6
            st.set_option("multi_attn_fast", 0)
            off = step_ms(st, B, P, reps)
            for s in range(B):                           # both settings step the same rows from the same position
                st.save_slot(s, P)
            st.set_option("multi_attn_fast", 1)
            on = step_ms(st, B, P, reps)
            st.set_option("multi_attn_fast", 0)
            for s in range(B):
                st.save_slot(s, P)
            log(f"{B:>4} {off:>12.3f} {on:>11.3f} {B / on * 1e3:>9.1f} {off / on:>9.2f}")
    if out_path:
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
