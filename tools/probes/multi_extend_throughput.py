"""Admission cost and mixed prefill + decode passes of the multi-token extend (kr_decode_extend_multi) on the 48-layer QCN synthetic (bench.build_qcn,
exact mode, E4M3 KV as bench's plain line) against the path that was the only one before it -- the store's own prompt pass, then save_slot --
measured in the same run.

Admission: a 512- and a 4096-token prompt into an empty slot.  Before: reset_decode_state + prefill + save_slot (clobbers the store's sequence; the
copy starts with a device synchronise).  Now: prefill_slot (extend_multi over chunks of KR_EXTEND_MAX_TOKENS).  Mixed pass: 63 decode rows at position
512 plus one 256-token prompt chunk.  Before: a 63-row step_multi, then reset + prefill of the 256 tokens + save_slot.  Now: one extend_multi of 64
rows.  Median wall time of the timed repeats after warm-up; every call returns after its ids are back on the host.  --profile: only mixed
extend_multi passes (for a rocprofv3 --kernel-trace --stats run of its own).

    python tools/probes/multi_extend_throughput.py [out.txt] [--profile]

--flash: the "multi_extend_flash" option (docs/design/25-multi-extend-flash.md) against the exact run kernels instead.  Admission of a 512- and a 4096-token
prompt with prefill_slot and the mixed pass, on flat slots and on pages of 64 positions; option off and option on alternate call by call inside this process;
the median of the timed calls after warm-up per leg; three rounds, every round's medians and their spread are reported.  --flash --off-only: the off leg alone
and no option call (a library built from another commit, loaded through KRASIS_HIP_LIB: has option off moved?).  --flash --profile: six mixed passes on flat
slots and nothing else, option on (with --off-only: off; with --admission: one 4096-token admission instead), for a rocprofv3 --kernel-trace --stats run.

    python tools/probes/multi_extend_throughput.py [out.txt] --flash [--off-only] [--profile [--admission]]

--la-chunk: the same legs for the "multi_extend_la_chunk" option (docs/design/26-multi-extend-la-chunk.md): "multi_extend_flash" stays on throughout and the
new option alternates off and on call by call.  --off-only, --profile and --admission as under --flash (--off-only never names the new option, so it also runs
against a library built from the commit before it).

    python tools/probes/multi_extend_throughput.py [out.txt] --la-chunk [--off-only] [--profile [--admission]]

--mla-flash: the same legs for the "multi_extend_mla_flash" option (docs/design/27-multi-extend-mla-flash.md) on the 27-layer V2-Lite synthetic
(bench.build_v2lite, MLA layers, E4M3 latent caches): the option alternates off and on call by call.  --off-only, --profile and --admission as under --flash.

    python tools/probes/multi_extend_throughput.py [out.txt] --mla-flash [--off-only] [--profile [--admission]]

--exact-mfma: the same legs for the "multi_extend_exact_mfma" option (docs/design/28-multi-extend-exact-mfma.md), which changes no bit: the option alternates
off and on call by call.  Two more legs, where the query tiles are mostly empty: the 63 decode slots each take a run of 2, and of 8, tokens at position 512.
--off-only, --profile and --admission as under --flash.

    python tools/probes/multi_extend_throughput.py [out.txt] --exact-mfma [--off-only] [--profile [--admission]]

--mla-exact-mfma: the legs of --exact-mfma, the two short-run legs included, for the "multi_extend_mla_exact_mfma" option
(docs/design/29-multi-extend-mla-exact-mfma.md) on the 27-layer V2-Lite synthetic (bench.build_v2lite, MLA layers, E4M3 latent caches): no bit changes, the
option alternates off and on call by call.  --off-only, --profile and --admission as under --flash.

    python tools/probes/multi_extend_throughput.py [out.txt] --mla-exact-mfma [--off-only] [--profile [--admission]]

--la-exact: the legs of --exact-mfma for the "multi_extend_la_exact" option (docs/design/36-multi-extend-la-exact.md), which changes no bit:
"multi_extend_exact_mfma" stays on throughout, "multi_extend_la_exact_min" is 2 so that every run of the short-run legs is staged, and the new option
alternates off and on call by call.  The short-run legs: the 63 decode slots each take a run of 2, 8 and 16 tokens at position 512, and one slot alone takes a
run of 2, 8, 16 and 64 tokens there -- what the default of the threshold is read from.  --off-only, --profile and --admission as under --flash (--off-only
never names the new options, so it also runs against a library built from the commit before them).

    python tools/probes/multi_extend_throughput.py [out.txt] --la-exact [--off-only] [--profile [--admission]]
"""
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

import bench  # noqa: E402

P_DECODE, N_DECODE, CHUNK = 512, 63, 256
PROMPTS = (512, 4096)


def timed(fn, warm, reps):
    ts = []
    for i in range(warm + reps):
        t0 = time.perf_counter(); fn(i); ts.append(time.perf_counter() - t0)
    return statistics.median(ts[warm:])


def flash_legs(out_path, off_only, profile, opt="multi_extend_flash", fixed=(), v2lite=False, short_runs=(), single_runs=(), opt_values=()):
    """option `opt` off / on, alternating call by call: admission (prefill_slot) and the mixed pass, flat and paged; the options of `fixed` stay on"""
    kv = 4096 + 160
    eng, st, keep = bench.build_v2lite(0, 0, 27, rope_len=kv, kv_fp8=True) if v2lite else bench.build_qcn(0, 0, 48, rope_len=kv, kv_fp8=True)
    lines = []

    def log(s):
        print(s, flush=True); lines.append(s)
        if out_path:
            with open(out_path, "w") as f:
                f.write("\n".join(lines) + "\n")

    toks = lambda n, i=0: [(i * 131 + j * 7) % 1000 for j in range(n)]
    nslots, adm, chunk_slot = N_DECODE + 2, N_DECODE, N_DECODE + 1
    rows = list(range(N_DECODE))
    legs = (0,) if off_only else (0, 1)
    for f in fixed:
        st.set_option(f, 1)
    if not off_only:
        for name, value in opt_values:
            st.set_option(name, value)

    def option(v):
        if not off_only:
            st.set_option(opt, v)

    def alternate(fn, warm, reps):
        """fn(i) under option off and on in turn -> the median seconds of each leg's timed calls"""
        ts = {v: [] for v in legs}
        for i in range(warm + reps):
            for v in legs:
                option(v)
                t0 = time.perf_counter(); fn(i); dt = time.perf_counter() - t0
                if i >= warm:
                    ts[v].append(dt)
        option(0)
        return {v: statistics.median(t) for v, t in ts.items()}

    for paged in (False, True):
        kind = "pages of 64" if paged else "flat"
        pages = dict(page_tokens=64, n_pages=N_DECODE * ((P_DECODE + 64) // 64 + 1) + 2 * ((kv + 63) // 64)) if paged else {}
        log(f"slots ({kind}): {nslots} x {kv} positions, {st.create_slots(nslots, kv, **pages) / 2**30:.1f} GiB")
        st.fill_state_synthetic(kv, seed=99)
        for s in range(N_DECODE):
            st.save_slot(s, P_DECODE)

        def mixed(i):
            st.extend_multi(rows + [chunk_slot], [[(i * 7 + b) % 1000] for b in rows] + [toks(CHUNK, i)], [P_DECODE] * N_DECODE + [0])

        if profile:      # flat slots only: six mixed passes (--admission: one 4096-token admission instead), option on, or off with --off-only
            option(1)
            if "--admission" in sys.argv:
                st.prefill_slot(adm, toks(4096, 1))
            else:
                for i in range(6):
                    mixed(i)
            option(0)
            return
        cases = [("prompt 512 -> slot", lambda i: st.prefill_slot(adm, toks(512, i)), 1, 4), ("prompt 4096 -> slot", lambda i: st.prefill_slot(adm, toks(4096, i)), 1, 2),
                 (f"mixed: {N_DECODE} rows at {P_DECODE} + a {CHUNK}-token chunk", mixed, 2, 6)]
        for k in short_runs:      # every decode slot takes a run of k tokens at its position: query tiles that are mostly empty
            cases.append((f"{N_DECODE} runs of {k} tokens at {P_DECODE}", lambda i, k=k: st.extend_multi(rows, [toks(k, i + b) for b in rows], [P_DECODE] * N_DECODE), 2, 6))
        for k in single_runs:     # one decode slot alone takes a run of k tokens at its position
            cases.append((f"1 run of {k} tokens at {P_DECODE}", lambda i, k=k: st.extend_multi(rows[:1], [toks(k, i)], [P_DECODE]), 2, 6))
        for name, fn, warm, reps in cases:
            rounds = [alternate(fn, warm, reps) for _ in range(3)]
            for v in legs:
                ms = [r[v] * 1e3 for r in rounds]
                log(f"{kind:<12} {name:<44} option {v}: rounds {ms[0]:9.2f} {ms[1]:9.2f} {ms[2]:9.2f} ms   median {statistics.median(ms):9.2f}   spread {(max(ms) - min(ms)) / statistics.median(ms) * 100:5.1f} %")
            if len(legs) == 2:
                log(f"{kind:<12} {name:<44} on / off = {statistics.median([r[1] for r in rounds]) / statistics.median([r[0] for r in rounds]):.3f}")


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    out_path = args[0] if args else None
    profile = "--profile" in sys.argv
    if "--mla-flash" in sys.argv:
        return flash_legs(out_path, "--off-only" in sys.argv, profile, "multi_extend_mla_flash", v2lite=True)
    if "--mla-exact-mfma" in sys.argv:
        return flash_legs(out_path, "--off-only" in sys.argv, profile, "multi_extend_mla_exact_mfma", v2lite=True, short_runs=(2, 8))
    if "--exact-mfma" in sys.argv:
        return flash_legs(out_path, "--off-only" in sys.argv, profile, "multi_extend_exact_mfma", short_runs=(2, 8))
    if "--la-exact" in sys.argv:
        return flash_legs(out_path, "--off-only" in sys.argv, profile, "multi_extend_la_exact", ("multi_extend_exact_mfma",), short_runs=(2, 8, 16), single_runs=(2, 8, 16, 64),
                          opt_values=(("multi_extend_la_exact_min", 2),))
    if "--la-chunk" in sys.argv:
        return flash_legs(out_path, "--off-only" in sys.argv, profile, "multi_extend_la_chunk", ("multi_extend_flash",))
    if "--flash" in sys.argv:
        return flash_legs(out_path, "--off-only" in sys.argv, profile)
    kv = 4096 + 160
    eng, st, keep = bench.build_qcn(0, 0, 48, rope_len=kv, kv_fp8=True)
    lines = []

    def log(s):
        print(s, flush=True); lines.append(s)

    nslots = N_DECODE + 2
    log(f"slots: {nslots} x {kv} positions, {st.create_slots(nslots, kv) / 2**30:.1f} GiB")
    toks = lambda n, i=0: [(i * 131 + j * 7) % 1000 for j in range(n)]
    adm, chunk_slot = N_DECODE, N_DECODE + 1

    st.fill_state_synthetic(kv, seed=99)
    for s in range(N_DECODE):
        st.save_slot(s, P_DECODE)
    rows = list(range(N_DECODE))

    def mixed_new(i):
        st.extend_multi(rows + [chunk_slot], [[(i * 7 + b) % 1000] for b in rows] + [toks(CHUNK, i)], [P_DECODE + i] * N_DECODE + [0])

    def mixed_old(i):
        st.step_multi(rows, [(i * 7 + b) % 1000 for b in rows], [P_DECODE + 40 + i] * N_DECODE)
        st.reset_decode_state(kv); st.prefill(toks(CHUNK, i), 0); st.save_slot(chunk_slot, CHUNK)

    if profile:
        for i in range(6):
            mixed_new(i)
        return
    log(f"{'admission':<28} {'tokens':>7} {'before ms':>10} {'now ms':>10} {'now / before':>13}")
    for n in PROMPTS:
        def old(i):
            st.reset_decode_state(kv); st.prefill(toks(n, i), 0); st.save_slot(adm, n)

        def new(i):
            st.prefill_slot(adm, toks(n, i))

        reps = 6 if n <= 512 else 3
        t_old, t_new = timed(old, 2, reps), timed(new, 2, reps)
        log(f"{'prompt -> slot':<28} {n:>7} {t_old * 1e3:>10.2f} {t_new * 1e3:>10.2f} {t_new / t_old:>13.2f}")
    t_step = timed(lambda i: st.step_multi(rows, [(i * 7 + b) % 1000 for b in rows], [P_DECODE + 20 + i] * N_DECODE), 3, 8)
    t_old, t_new = timed(mixed_old, 3, 8), timed(mixed_new, 3, 8)
    log(f"{N_DECODE}-row step_multi alone at P = {P_DECODE}: {t_step * 1e3:.2f} ms")
    log(f"mixed pass, {N_DECODE} decode rows at P = {P_DECODE} + one {CHUNK}-token chunk: before (step_multi, then reset + prefill + save_slot) "
        f"{t_old * 1e3:.2f} ms, now (one extend_multi) {t_new * 1e3:.2f} ms, now / before {t_new / t_old:.2f}")
    log(f"decode rows stand still for: before {(t_old - t_step) * 1e3:.2f} ms per admitted chunk, now {(t_new - t_step) * 1e3:.2f} ms")
    if out_path:
        with open(out_path, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
