"""Q3_K experts (docs/design/47-gguf-q3k.md) on one MI355X at the shape a downloaded `Q3_K_M` file has: bench.py's QCN model with Q3_K gate | up and Q4_K
down, against the same model with Q4_K gate | up -- the nearest thing that existed before the type was served; Q3_K moves 112 / 144 of Q4_K's gate | up bytes.
Both models live in one process and are measured in alternating rounds, synthetic fill, E4M3 KV:

(a) decode_step rate of the exact step (runs of 100 steps after 10 warm-up steps): Q3_K is one f32 row chain per row, Q4_K an integer tile
(b) decode_step rate under KR_DECODE_FAST
(c) `prefill` of 8192 tokens under set_attention_mode(True, gemm_fast=True), bench.py's protocol (one un-timed pass, then 3 timed passes)
Every round's pair is printed, then the medians and ranges.

    python tools/probes/gguf_q3k.py [out.txt] [--layers N] [--tokens P]
"""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

import bench  # noqa: E402

ROUNDS = 3
NEW, OLD, DOWN = 11, 12, 12


def main():
    import torch
    from krasis_amd import KrasisEngine
    argv = sys.argv[1:]
    opt = lambda name, default: argv[argv.index(name) + 1] if name in argv else default
    layers, P = int(opt("--layers", 4)), int(opt("--tokens", 8192))
    args = [a for i, a in enumerate(argv) if not a.startswith("--") and (i == 0 or not argv[i - 1].startswith("--"))]
    lines = []

    def log(s):
        print(s, flush=True); lines.append(s)

    dims, kvm = bench.QCN, bench.QCN["kv_max_seq"]
    fill = KrasisEngine.fill_synthetic_gguf
    models = {}
    for gu_t in (NEW, OLD):
        KrasisEngine.fill_synthetic_gguf = lambda self, gate_up_type=12, down_type=12, seed=0, layers=None: fill(self, gu_t, DOWN, seed=seed, layers=layers)
        try:
            models[gu_t] = bench.build_qcn(0, 0, layers, rope_len=max(P, 1024) + 64, kv_fp8=True, gguf=True)
        finally:
            KrasisEngine.fill_synthetic_gguf = fill
    log(f"qcn, {layers} layers, Q4_K down; gate | up Q3_K (11) against Q4_K (12); byte ratio 112 / 144 = {112 / 144:.3f}")
    macs = bench.qcn_gemm_macs_per_token(layers)
    legs = (("(a) exact decode_step tok/s", lambda st: (st.set_attention_mode(False), 100 / bench.time_decode(st, 100, 10, kvm, torch, None, 1))[1]),
            ("(b) KR_DECODE_FAST decode_step tok/s", lambda st: (st.set_attention_mode(False, decode_fast=True), 100 / bench.time_decode(st, 100, 10, kvm, torch, None, 1))[1]),
            (f"(c) KR_GEMM_FAST prefill of {P} tokens, ms", lambda st: (st.set_attention_mode(True, gemm_fast=True), bench.prefill_model(st, dims, macs, layers, P, 3, torch)["ms"])[1]))
    for name, leg in legs:
        res = {NEW: [], OLD: []}
        for gu_t in (NEW, OLD):
            leg(models[gu_t][1])      # warm-up round, not recorded
        for r in range(ROUNDS):
            for gu_t in (NEW, OLD):
                res[gu_t].append(leg(models[gu_t][1]))
            log(f"{name} round {r}: Q3_K {res[NEW][-1]:9.2f}   Q4_K {res[OLD][-1]:9.2f}")
        m3, m4 = statistics.median(res[NEW]), statistics.median(res[OLD])
        log(f"{name}: Q3_K median {m3:.2f} (range {min(res[NEW]):.2f} .. {max(res[NEW]):.2f})   Q4_K median {m4:.2f} (range {min(res[OLD]):.2f} .. {max(res[OLD]):.2f})   Q3_K / Q4_K {m3 / m4:.3f}")
    if args:
        with open(args[0], "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
