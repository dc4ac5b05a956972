"""KR_GEMM_FAST prompt pass over Q6_K / Q5_0 experts read from their lane records (docs/design/42-gguf-fast-native.md) on one MI355X, at two shapes a
downloaded `Q4_K_M` file has: bench.py's QCN model with Q4_K gate | up and Q6_K down, and its V2-Lite model (I = 1408) with Q4_K gate | up and Q5_0 down.
Synthetic fill, E4M3 KV.  `prefill` of 2048 and of 8192 tokens under set_attention_mode(True, gemm_fast=True): bench.py's protocol (one un-timed pass, then
REPS timed passes; median and range).  `--down copy` measures the all-copy-form layer of the same shape instead (Q4_K down on QCN, Q8_0 down on V2-Lite).

The probe times ONE build of the library per process.  To compare two builds, run it once per build and round, alternating, KRASIS_HIP_LIB naming the
other one; every process appends its lines to out.txt.

    python tools/probes/gguf_fast_native.py [out.txt] [--layers N] [--shape qcn|v2lite] [--down native|copy] [--tokens P] [--tag NAME]
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

import bench  # noqa: E402

REPS = 3
SHAPES = {"qcn": (bench.build_qcn, bench.QCN, 14, 12, bench.qcn_gemm_macs_per_token), "v2lite": (bench.build_v2lite, bench.V2L, 6, 8, bench.v2l_gemm_macs_per_token)}


def main():
    import torch
    from krasis_amd import KrasisEngine
    argv = sys.argv[1:]
    opt = lambda name, default: argv[argv.index(name) + 1] if name in argv else default
    layers, down, tag = int(opt("--layers", 4)), opt("--down", "native"), opt("--tag", os.environ.get("KRASIS_HIP_LIB", "default"))
    shapes = [opt("--shape", None)] if "--shape" in argv else list(SHAPES)
    tokens = [int(opt("--tokens", 0))] if "--tokens" in argv else [2048, 8192]
    args = [a for i, a in enumerate(argv) if not a.startswith("--") and (i == 0 or not argv[i - 1].startswith("--"))]
    lines = []
    for shape in shapes:
        build, dims, native_t, copy_t, macs = SHAPES[shape]
        down_t = native_t if down == "native" else copy_t
        fill = KrasisEngine.fill_synthetic_gguf
        KrasisEngine.fill_synthetic_gguf = lambda self, gate_up_type=12, down_type=12, seed=0, layers=None: fill(self, 12, down_t, seed=seed, layers=layers)
        try:
            eng, st, keep = build(0, 0, layers, rope_len=max(tokens) + 64, kv_fp8=True, gguf=True)
        finally:
            KrasisEngine.fill_synthetic_gguf = fill
        st.set_attention_mode(True, gemm_fast=True)
        for P in tokens:
            r = bench.prefill_model(st, dims, macs(layers), layers, P, REPS, torch)
            ms = r["ms_all"]
            lines.append(f"{shape} Q4_K gate | up, type {down_t} down, {layers} layers, {P} tokens, library {tag}: median {r['value']:.0f} tok/s ({r['ms']:.2f} ms)   "
                         f"range {min(ms):.2f} .. {max(ms):.2f} ms   n {len(ms)}   allocs {r['allocs_in_timed_region']}")
            print(lines[-1], flush=True)
        del eng, st, keep
        torch.cuda.empty_cache()
    if args:
        with open(args[0], "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
