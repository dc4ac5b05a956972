"""The exact pass over native GGUF experts (kr_decode_set_option "gguf_exact_pass", docs/design/20-gguf-exact-pass.md) on bench.py's `qcn-q4k-gguf`
shape (bench.build_qcn(gguf=True): hidden 2048, expert intermediate 512, 512 experts, top 10, Q4_K gate / up / down, E4M3 KV).

(a) prefill of 2048 tokens: option off (the int8-MFMA tolerance form), option on (the grouped kernels), option on with "gguf_exact_grouped" 0 (the
    streaming kernels).  One un-timed pass per setting, then the settings alternate; median and range of the timed passes.
(b) step_multi at B = 16 and 64, every slot at position 512: option on, grouped 1 against grouped 0, alternating; median and range.
(c) --decode: only the single-sequence decode_step rate (runs of 100 steps after 10 warm-up steps, median and range), for a comparison of two builds of
    the library (KRASIS_HIP_LIB names the other build): the streaming kernels share a header with the grouped ones.
--profile: a few B = 64 steps with the grouped kernels only (for a rocprofv3 --kernel-trace --stats run of its own).

    python tools/probes/gguf_exact_pass.py [out.txt] [--layers N] [--decode] [--profile]
"""
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

import bench  # noqa: E402

P_TOKENS = 2048
POS = 512
SETTINGS = (("off (int8 MFMA, tolerance)", 0, 1), ("on, grouped", 1, 1), ("on, streaming", 1, 0))


def fmt(ts):
    return f"median {statistics.median(ts):9.2f} ms   range {min(ts):9.2f} .. {max(ts):9.2f}   n {len(ts)}"


def main():
    import numpy as np
    import torch
    argv = sys.argv[1:]
    layers = int(argv[argv.index("--layers") + 1]) if "--layers" in argv else bench.QCN["layers"]
    flags = {a for a in argv if a.startswith("--")}
    args = [a for i, a in enumerate(argv) if not a.startswith("--") and (i == 0 or argv[i - 1] != "--layers")]
    out_path = args[0] if args else None
    kv = P_TOKENS + 64
    eng, st, keep = bench.build_qcn(0, 0, layers, rope_len=kv, kv_fp8=True, gguf=True)
    lines = []

    def log(s):
        print(s, flush=True); lines.append(s)

    def select(exact, grouped):
        st.set_option("gguf_exact_pass", exact); st.set_option("gguf_exact_grouped", grouped)

    log(f"qcn-q4k-gguf, {layers} layers, library {os.environ.get('KRASIS_HIP_LIB', 'default')}")
    if "--decode" in flags:
        rates = []
        for _ in range(7):
            dt = bench.time_decode(st, 100, 10, bench.QCN["kv_max_seq"], torch, None, 1)
            rates.append(100 / dt)
        log(f"(c) decode_step tok/s: median {statistics.median(rates):.1f}   range {min(rates):.1f} .. {max(rates):.1f}   n {len(rates)}")
    else:
        select(1, 1)                                            # the slot copies refuse a GGUF store without the option
        st.create_slots(64, kv)
        st.fill_state_synthetic(kv, seed=99)
        for s in range(64):
            st.save_slot(s, POS)

        def step_ms(B, i):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            st.step_multi(list(range(B)), [(i * 7 + b) % 1000 for b in range(B)], [POS + (i % 32)] * B)      # returns after the ids' read-back
            return (time.perf_counter() - t0) * 1e3

        if "--profile" in flags:
            select(1, 1)
            for i in range(6):
                step_ms(64, i)
            return
        toks = [int(x) for x in np.random.default_rng(5).integers(0, bench.QCN["vocab"], P_TOKENS)]

        def prefill_ms():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            st.prefill(toks, 0)
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3

        times = {name: [] for name, _, _ in SETTINGS}
        for name, exact, grouped in SETTINGS:                    # warm-up: every arena and derived table of every setting exists
            select(exact, grouped); prefill_ms()
        for _ in range(3):
            for name, exact, grouped in SETTINGS:
                select(exact, grouped); times[name].append(prefill_ms())
        log(f"(a) prefill of {P_TOKENS} tokens")
        for name, _, _ in SETTINGS:
            log(f"    {name:<28} {fmt(times[name])}   {P_TOKENS / statistics.median(times[name]) * 1e3:9.0f} tok/s")
        log(f"(b) step_multi at position {POS}")
        for B in (16, 64):
            ts = {1: [], 0: []}
            for grouped in (1, 0):
                select(1, grouped)
                for i in range(3):
                    step_ms(B, i)
            for i in range(10):
                for grouped in (1, 0):
                    select(1, grouped); ts[grouped].append(step_ms(B, i))
            log(f"    B = {B:<3} grouped    {fmt(ts[1])}   {B / statistics.median(ts[1]) * 1e3:8.0f} tok/s")
            log(f"    B = {B:<3} streaming  {fmt(ts[0])}   {B / statistics.median(ts[0]) * 1e3:8.0f} tok/s")
        select(0, 1)
    if out_path:
        with open(out_path, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
