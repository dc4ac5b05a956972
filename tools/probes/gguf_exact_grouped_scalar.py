"""The exact pass on layers that hold a Q6_K / Q5_0 matrix (docs/design/43-gguf-exact-grouped-scalar.md) on one MI355X, at two shapes a downloaded `Q4_K_M`
file has: bench.py's QCN model with Q4_K gate | up and Q6_K down, and its V2-Lite model (I = 1408) with Q4_K gate | up and Q5_0 down; 4 layers, E4M3 KV,
"gguf_exact_pass" on.  Legs: step_multi of 16 and of 64 rows at position 512 (the call returns after the ids' read-back), prefill of 2048 tokens (timed to a
device synchronise).

Two builds of the library are compared in one call: this tree's and the one --other names (the parent commit's).  Every visit is a fresh process (a library is
chosen at import, KRASIS_HIP_LIB); the visits alternate other / this for ROUNDS rounds per shape.  A process on this tree's build times
"gguf_exact_grouped_scalar" 1 and 0 alternately, after un-timed passes of each.  The table gives the median and the range over all timed passes of a leg, and the
medians of the single visits (their spread is the noise a difference has to exceed).  The last token of every prefill must agree across all of them.

    python tools/probes/gguf_exact_grouped_scalar.py --other /path/to/parent/libkrasis_hip.so [out.txt]
    python tools/probes/gguf_exact_grouped_scalar.py --profile qcn|v2lite      (a few passes of every leg with the option on: for rocprofv3 --kernel-trace --stats)
"""
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

ROUNDS, LAYERS, POS, P_TOKENS = 3, 4, 512, 2048
N_STEP, N_PREFILL = 10, 3
SHAPES = {"qcn": ("build_qcn", "QCN", 12, 14), "v2lite": ("build_v2lite", "V2L", 12, 6)}      # bench.py builder, its dims, ggml types of gate | up and of down
SCRIPT = os.path.abspath(__file__)      # what a visit runs: a probe that brings other SHAPES (gguf_q5k_grouped.py) names itself
LEGS = ("step_multi 16 rows", "step_multi 64 rows", f"prefill {P_TOKENS} tokens")


def visit(shape, profile=False):
    """one process, one library: {leg: {option: [ms]}} and the prefills' last tokens as one JSON line"""
    import numpy as np
    import torch
    import bench
    from krasis_amd import KrasisEngine
    build, dims, gu_t, down_t = SHAPES[shape]
    fill = KrasisEngine.fill_synthetic_gguf
    KrasisEngine.fill_synthetic_gguf = lambda self, gate_up_type=12, down_type=12, **kw: fill(self, gu_t, down_t, **kw)      # bench.py's model with other block types
    try:
        eng, st, keep = getattr(bench, build)(0, 0, LAYERS, rope_len=P_TOKENS + 64, kv_fp8=True, gguf=True)
    finally:
        KrasisEngine.fill_synthetic_gguf = fill
    st.set_option("gguf_exact_pass", 1)
    try:
        st.set_option("gguf_exact_grouped_scalar", 1); options = (1,) if profile else (1, 0)
    except ValueError:                                       # the build from before the option
        options = ("-",)
    select = lambda o: st.set_option("gguf_exact_grouped_scalar", o) if o != "-" else None
    st.create_slots(64, P_TOKENS + 64)
    st.fill_state_synthetic(P_TOKENS + 64, seed=99)
    for s in range(64):
        st.save_slot(s, POS)
    toks = [int(x) for x in np.random.default_rng(5).integers(0, getattr(bench, dims)["vocab"], P_TOKENS)]
    last = []

    def step_ms(B, i):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        st.step_multi(list(range(B)), [(i * 7 + b) % 1000 for b in range(B)], [POS + (i % 32)] * B)
        return (time.perf_counter() - t0) * 1e3

    def prefill_ms(_):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        st.prefill(toks, 0)
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) * 1e3
        last.append(st.last_token())
        return dt

    out = {}
    for leg, call, warm, n in ((LEGS[0], lambda i: step_ms(16, i), 3, N_STEP), (LEGS[1], lambda i: step_ms(64, i), 3, N_STEP), (LEGS[2], prefill_ms, 1, N_PREFILL)):
        ts = {str(o): [] for o in options}
        for o in options:
            select(o)
            for i in range(warm):
                call(i)
        for i in range(2 if profile else n):
            for o in options:
                select(o); ts[str(o)].append(call(i))
        out[leg] = ts
    print("VISIT " + json.dumps(dict(times=out, last=last)), flush=True)


def main():
    argv = sys.argv[1:]
    if "--visit" in argv:
        return visit(argv[argv.index("--visit") + 1])
    if "--profile" in argv:
        return visit(argv[argv.index("--profile") + 1], profile=True)
    other = argv[argv.index("--other") + 1]
    args = [a for i, a in enumerate(argv) if not a.startswith("--") and (i == 0 or argv[i - 1] != "--other")]
    lines = []

    def log(s):
        print(s, flush=True); lines.append(s)

    for shape in SHAPES:
        cols = {}      # column -> leg -> list of per-visit lists
        lasts = set()
        for r in range(ROUNDS):
            for lib in (other, None):
                env = dict(os.environ)
                env.pop("KRASIS_HIP_LIB", None)
                if lib:
                    env["KRASIS_HIP_LIB"] = lib
                p = subprocess.run([sys.executable, SCRIPT, "--visit", shape], env=env, capture_output=True, text=True, timeout=240)
                if p.returncode:      # nothing more on the GPU after a visit that failed
                    sys.exit(f"visit {shape} round {r} library {lib or 'this tree'} ended with {p.returncode}\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}")
                res = json.loads(next(ln for ln in p.stdout.splitlines() if ln.startswith("VISIT "))[6:])
                lasts.update(res["last"])
                for leg, ts in res["times"].items():
                    for o, v in ts.items():
                        col = "parent build" if lib else f"this tree, option {o}"
                        cols.setdefault(col, {}).setdefault(leg, []).append(v)
        log(f"{shape}: type {SHAPES[shape][2]} gate | up, type {SHAPES[shape][3]} down, {LAYERS} layers, E4M3 KV, gguf_exact_pass; {ROUNDS} rounds of alternating processes; last token of every prefill: {sorted(lasts)}")
        assert len(lasts) == 1, lasts
        for leg in LEGS:
            for col in sorted(cols):
                visits = cols[col][leg]
                every = [t for v in visits for t in v]
                log(f"    {leg:<20} {col:<22} median {statistics.median(every):8.2f} ms   range {min(every):8.2f} .. {max(every):8.2f}   n {len(every):<3} "
                    f"medians of the visits {' '.join(f'{statistics.median(v):.2f}' for v in visits)}")
    if args:
        with open(args[0], "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
