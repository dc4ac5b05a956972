"""Cost of per-row sampling in the multi-sequence step (kr_decode_step_multi_sample) on the 48-layer QCN synthetic (bench.build_qcn, exact mode,
E4M3 KV as bench's plain line), every slot at position P = 512 with fill_state_synthetic's state.

Per B in (1, 8, 64, 256): the median wall time of step_multi (greedy), step_multi_sample with the server defaults (temperature 0.6, top_k 50,
top_p 0.95) on the batched kernels, and the same with kr_decode_set_option("multi_sample_loop", 1) (the single-row sampler once per row),
interleaved call by call.  Then generate_multi at B = 64, greedy against sampled.  --profile: only sampled B = 64 steps (for a
rocprofv3 --kernel-trace --stats run of its own).

    python tools/probes/multi_sample_cost.py [out.txt] [--profile]
"""
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

import bench  # noqa: E402

BS = (1, 8, 64, 256)
P = 512
SERVER = (0.6, 50, 0.95, 0.0)     # temperature, top_k, top_p, presence_penalty


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    out_path = args[0] if args else None
    profile = "--profile" in sys.argv
    kv = P + 160
    eng, st, keep = bench.build_qcn(0, 0, 48, rope_len=kv, kv_fp8=True)
    lines = []

    def log(s):
        print(s, flush=True); lines.append(s)

    nslots = 64 if profile else max(BS)
    log(f"slots: {nslots} x {kv} positions, {st.create_slots(nslots, kv) / 2**30:.1f} GiB; P = {P}; sampled = {SERVER}")
    st.fill_state_synthetic(kv, seed=99)
    for s in range(nslots):
        st.save_slot(s, P)
        st.set_slot_sampler(s, s % 1000, *SERVER, rng_seed=s + 1)
    if profile:
        for i in range(6):
            st.step_multi_sample(list(range(64)), [i] * 64, [P + i] * 64)
        return
    log(f"{'B':>4} {'greedy ms':>10} {'sampled ms':>11} {'x greedy':>9} {'loop ms':>9} {'loop/batched extra':>19}")
    for B in BS:
        reps = 12 if B <= 64 else 8
        tg, ts, tl = [], [], []
        for i in range(reps + 3):
            sl, tk, ps = list(range(B)), [(i * 7 + b) % 1000 for b in range(B)], [P + i % 100] * B
            t0 = time.perf_counter(); st.step_multi(sl, tk, ps); tg.append(time.perf_counter() - t0)
            t0 = time.perf_counter(); st.step_multi_sample(sl, tk, ps); ts.append(time.perf_counter() - t0)
            st.set_option("multi_sample_loop", 1)
            t0 = time.perf_counter(); st.step_multi_sample(sl, tk, ps); tl.append(time.perf_counter() - t0)
            st.set_option("multi_sample_loop", 0)
        g, s_, l_ = (statistics.median(x[3:]) for x in (tg, ts, tl))
        extra = (l_ - g) / (s_ - g) if s_ > g else float("inf")
        log(f"{B:>4} {g * 1e3:>10.3f} {s_ * 1e3:>11.3f} {s_ / g:>9.4f} {l_ * 1e3:>9.3f} {extra:>19.1f}")
    n_tok = 24
    for name, kw in (("greedy", {}), ("sampled", dict(temperature=SERVER[0], top_k=SERVER[1], top_p=SERVER[2], presence_penalty=SERVER[3],
                                                        rng_seeds=list(range(1, 65))))):
        for s in range(64):
            st.save_slot(s, P)
        t0 = time.perf_counter()
        outs = st.generate_multi(list(range(64)), [b % 1000 for b in range(64)], [P] * 64, n_tok, **kw)
        t = time.perf_counter() - t0
        log(f"generate_multi B = 64, {n_tok} tokens per row, {name}: {sum(len(o) for o in outs) / t:.1f} tok/s")
    if out_path:
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
