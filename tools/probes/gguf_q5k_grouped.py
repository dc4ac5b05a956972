"""The exact pass on layers with Q5_K experts (docs/design/46-gguf-q5k-grouped.md) on one MI355X: bench.py's QCN model cut to 4 layers, E4M3 KV, synthetic
weights, "gguf_exact_pass" on, with the two layer flavours of a `Q5_K_M` file -- Q5_K gate | up with Q6_K down, and Q5_K gate | up with Q5_K down.

The harness, the legs and the table are those of gguf_exact_grouped_scalar.py (this tree's library against the parent commit's, fresh processes alternating for
three rounds after un-timed passes, "gguf_exact_grouped_scalar" 1 and 0 alternately inside a process): this file only names the stores.  The parent build
streams these layers under either option value, so its column holds both.

    python tools/probes/gguf_q5k_grouped.py --other /path/to/parent/libkrasis_hip.so [out.txt]
    python tools/probes/gguf_q5k_grouped.py --profile q5k-q6k|q5k-q5k      (a few passes of every leg with the option on: for rocprofv3 --kernel-trace --stats)
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gguf_exact_grouped_scalar as probe  # noqa: E402

probe.SHAPES = {"q5k-q6k": ("build_qcn", "QCN", 13, 14), "q5k-q5k": ("build_qcn", "QCN", 13, 13)}
probe.SCRIPT = os.path.abspath(__file__)

if __name__ == "__main__":
    probe.main()
