"""Q5_0 / Q6_K experts on the lane-record layout and their f32 tiles (docs/design/41-gguf-scalar-tiles.md) on one MI355X, at two shapes a downloaded
`Q4_K_M` file has: bench.py's QCN model with Q4_K gate | up and Q6_K down, and its V2-Lite model (I = 1408) with Q4_K gate | up and Q5_0 down.

(a) decode_step rate under KR_DECODE_FAST with "gguf_scalar_tiles" 0 and 1, alternating in one process: ROUNDS rounds of runs of 100 steps after 10
    warm-up steps; every round's pair is printed, the option's default rests on all of them.  Skipped on a library without the option.
(b) decode_step rate of the exact step (runs of 100 steps, median and range).
(c) step_multi of 16 rows at position 512 under "gguf_exact_pass" (ms per call, median and range).
(b) and (c) compare two builds of the library: run the probe once per build, KRASIS_HIP_LIB naming the other one.  A build whose synthetic fill does not
know the two types gets one host-generated expert per layer uploaded into every expert slot (same bytes in every expert: timing only).

    python tools/probes/gguf_scalar_tiles.py [out.txt] [--layers N] [--shape qcn|v2lite]
"""
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

import bench  # noqa: E402

ROUNDS, POS, ROWS = 5, 512, 16
SHAPES = {"qcn": (bench.build_qcn, bench.QCN, 14, 210, 256), "v2lite": (bench.build_v2lite, bench.V2L, 6, 22, 32)}


def main():
    import numpy as np
    import torch
    from krasis_amd import KrasisEngine
    argv = sys.argv[1:]
    layers = int(argv[argv.index("--layers") + 1]) if "--layers" in argv else 8
    shapes = [argv[argv.index("--shape") + 1]] if "--shape" in argv else list(SHAPES)
    args = [a for i, a in enumerate(argv) if not a.startswith("--") and (i == 0 or not argv[i - 1].startswith("--"))]
    lines = []

    def log(s):
        print(s, flush=True); lines.append(s)

    for shape in shapes:
        build, dims, down_t, down_bb, down_be = SHAPES[shape]
        H, I, E = dims["hidden"], dims["inter"], dims["experts"]
        fill = KrasisEngine.fill_synthetic_gguf

        def fill_mixed(self, gate_up_type=12, down_type=12, seed=0, layers=None):      # the model of bench.py with another down type
            try:
                fill(self, 12, down_t, seed=seed, layers=layers)
            except ValueError:                                                         # a build from before the types' synthetic fill
                rng = np.random.default_rng(seed % 2**32)
                raw = lambda rows, nb, bb: rng.integers(0, 256, (rows, nb * bb), dtype=np.uint8)
                for layer in range(self._cfg.num_moe_layers):
                    g, u, d = raw(I, H // 256, 144), raw(I, H // 256, 144), raw(H, I // down_be, down_bb)
                    for m, nb, bb, off in ((g, H // 256, 144, 0), (u, H // 256, 144, 0), (d, I // down_be, down_bb, 208 if down_t == 14 else 0)):
                        v = m.reshape(m.shape[0], nb, bb); v[:, :, off] = 0x66; v[:, :, off + 1] = 0x10      # d = f16 bits 0x1066 (6.4e-4) in every block
                        if bb == 144:
                            v[:, :, 2] = 0x66; v[:, :, 3] = 0x0C                                             # Q4_K dmin
                    for e in range(E):
                        self.load_gguf_expert(layer, e, g, u, d, 12, down_t, I)

        KrasisEngine.fill_synthetic_gguf = fill_mixed
        try:
            eng, st, keep = build(0, 0, layers, rope_len=1024 + 64, kv_fp8=True, gguf=True)
        finally:
            KrasisEngine.fill_synthetic_gguf = fill
        kvm = dims["kv_max_seq"]
        log(f"{shape}: Q4_K gate | up, type {down_t} down, {layers} layers, library {os.environ.get('KRASIS_HIP_LIB', 'default')}")

        def rate():
            return 100 / bench.time_decode(st, 100, 10, kvm, torch, None, 1)

        try:
            st.set_option("gguf_scalar_tiles", 1); has_opt = True
        except ValueError:
            has_opt = False
        if has_opt:
            st.set_attention_mode(False, decode_fast=True)
            for v in (0, 1):
                st.set_option("gguf_scalar_tiles", v); rate()
            for r in range(ROUNDS):
                pair = []
                for v in (0, 1):
                    st.set_option("gguf_scalar_tiles", v); pair.append(rate())
                log(f"(a) round {r}: KR_DECODE_FAST decode_step tok/s   option 0 {pair[0]:8.1f}   option 1 {pair[1]:8.1f}")
            st.set_attention_mode(False)
        rates = [rate() for _ in range(1 + ROUNDS)][1:]
        log(f"(b) exact decode_step tok/s: median {statistics.median(rates):.1f}   range {min(rates):.1f} .. {max(rates):.1f}   n {len(rates)}")
        try:
            st.set_option("gguf_exact_pass", 1)
            st.create_slots(ROWS, POS + 64)
            st.fill_state_synthetic(POS + 64, seed=99)
            for s in range(ROWS):
                st.save_slot(s, POS)
            ms = []
            for i in range(3 + 2 * ROUNDS):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                st.step_multi(list(range(ROWS)), [(i * 7 + b) % 1000 for b in range(ROWS)], [POS + (i % 32)] * ROWS)      # returns after the ids' read-back
                ms.append((time.perf_counter() - t0) * 1e3)
            ms = ms[3:]
            log(f"(c) step_multi of {ROWS} rows under gguf_exact_pass: median {statistics.median(ms):.2f} ms   range {min(ms):.2f} .. {max(ms):.2f}   n {len(ms)}")
        except (ValueError, RuntimeError) as ex:
            log(f"(c) step_multi of {ROWS} rows under gguf_exact_pass: not run ({ex})")
        del eng, st, keep
        torch.cuda.empty_cache()
    if args:
        with open(args[0], "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
