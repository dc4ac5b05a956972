"""Aggregate throughput of the exact multi-sequence decode step (kr_decode_step_multi) on the 48-layer QCN synthetic (bench.build_qcn, exact mode,
E4M3 KV as bench's plain line) against the single-sequence exact step measured in the same run.

Every slot holds the fill_state_synthetic state saved at position P (512, 4096).  Per B: the median wall time of one step_multi after warm-up (it
returns after the ids' read-back), the aggregate tok/s B / t, and the ratio to the plain step (decode_step + last_token).  Then generate_multi at
B = 64.  --profile: only B = 64 steps at P = 512 (for a rocprofv3 --kernel-trace --stats run of its own).

--page-tokens N: the slots are paged (create_slots(..., page_tokens=N, n_pages=...), docs/design/21-paged-slots.md) with a pool sized for the run --
every slot to the longest position the run reaches, or --pages M; several values (N1,N2,0; 0 = flat) are measured ALTERNATELY per (P, B), slots
re-created for each, so flat and paged share one process and one warm device.  --bs / --ps restrict the batch sizes and positions, --rounds R repeats
each (P, B, geometry) measurement R times (every median is printed: their spread is the noise).

    python tools/probes/multi_seq_throughput.py [out.txt] [--profile] [--page-tokens 64,256,0] [--pages M] [--bs 64,256] [--ps 512,4096] [--rounds 3]
"""
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

import bench  # noqa: E402

BS = (1, 2, 4, 8, 16, 32, 64, 128, 256)
PS = (512, 4096)


def _opt(name, default=None):
    """--name value -> value (and both leave sys.argv)"""
    if name not in sys.argv:
        return default
    i = sys.argv.index(name)
    v = sys.argv[i + 1]
    del sys.argv[i:i + 2]
    return v


def paged_run(st, kv, geoms, pages, bs, ps, rounds, log):
    """flat (0) and paged geometries alternately per (P, B): slots re-created and filled for each measurement"""
    nslots = max(bs)
    reach = max(ps) + 64                                   # the longest position a slot reaches in this run
    for g in geoms:
        n_pages = pages or nslots * ((reach + g - 1) // g) if g else 0
        gib = st.create_slots(nslots, kv, **(dict(page_tokens=g, n_pages=n_pages) if g else {})) / 2**30
        log(f"{'flat' if not g else f'page_tokens {g}, {n_pages} pages'}: {nslots} slots x {kv} positions, {gib:.2f} GiB")
    log(f"{'P':>5} {'B':>4} {'geometry':>10} {'ms/step (median of 12, per round)':>36}")
    for P in ps:
        for B in bs:
            meds = {g: [] for g in geoms}
            for r in range(rounds):
                for g in geoms:
                    n_pages = pages or nslots * ((reach + g - 1) // g) if g else 0
                    st.create_slots(B, kv, **(dict(page_tokens=g, n_pages=n_pages) if g else {}))
                    st.fill_state_synthetic(kv, seed=99)
                    for s in range(B):
                        st.save_slot(s, P)
                    ts = []
                    for i in range(15):
                        t0 = time.perf_counter()
                        st.step_multi(list(range(B)), [(i * 7 + b) % 1000 for b in range(B)], [P + i] * B)
                        ts.append(time.perf_counter() - t0)
                    meds[g].append(statistics.median(ts[3:]) * 1e3)
            for g in geoms:
                log(f"{P:>5} {B:>4} {('flat' if not g else f'paged {g}'):>10}   " + "  ".join(f"{m:8.3f}" for m in meds[g]))


def main():
    page_tokens = _opt("--page-tokens")
    pages = int(_opt("--pages", 0))
    bs = tuple(int(x) for x in _opt("--bs", ",".join(map(str, BS))).split(","))
    ps = tuple(int(x) for x in _opt("--ps", ",".join(map(str, PS))).split(","))
    rounds = int(_opt("--rounds", 1))
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    out_path = args[0] if args else None
    profile = "--profile" in sys.argv
    kv = 4096 + 160
    eng, st, keep = bench.build_qcn(0, 0, 48, rope_len=kv, kv_fp8=True)
    lines = []

    def log(s):
        print(s, flush=True); lines.append(s)

    if page_tokens is not None:
        paged_run(st, kv, [int(x) for x in page_tokens.split(",")], pages, bs, ps, rounds, log)
        if out_path:
            with open(out_path, "w") as f:
                f.write("\n".join(lines) + "\n")
        return
    nslots = 64 if profile else max(bs)
    log(f"slots: {nslots} x {kv} positions, {st.create_slots(nslots, kv) / 2**30:.1f} GiB")
    for P in ((512,) if profile else ps):
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
        for B in bs:
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
        if P == 512 and nslots >= 64:
            for s in range(64):
                st.save_slot(s, P)
            n_tok = 24
            t0 = time.perf_counter()
            outs = st.generate_multi(list(range(64)), [b % 1000 for b in range(64)], [P] * 64, n_tok)
            t = time.perf_counter() - t0
            log(f"generate_multi B = 64, {n_tok} tokens per row: {sum(len(o) for o in outs) / t:.1f} tok/s")
    if out_path:
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
