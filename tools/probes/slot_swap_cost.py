"""What moving a slot between the device and host memory costs (kr_decode_slots_export / kr_decode_slots_import, docs/design/38-slot-swap.md), on the 48-layer
QCN synthetic (bench.build_qcn) and the V2-Lite synthetic (bench.build_v2lite), exact mode, E4M3 caches.

For one slot and for 16 slots at 512 and 4096 positions, in pages of 64 and flat:
  * kr_decode_slots_export and kr_decode_slots_import into and out of image buffers allocated and touched beforehand (a caller that swaps keeps its buffers;
    CpuDecodeStore.export_slots allocates fresh arrays, whose first touch would be timed with the copy), wall ms and GB/s, for every "slot_swap_chunk_bytes" of 1, 4, 16, 64 and 256 MiB (median of --reps calls after one of warm-up,
    which also allocates the staging buffers); the images that come back are compared with the first ones;
  * the ceiling: one plain pinned copy of the same byte count in each direction (torch, pinned host tensor <-> device tensor);
  * the floor: the route without this feature, load_slot + get_decode_state of every layer for every slot (pageable copies; get_decode_state returns the store's
    whole kv_max_seq rows, here the slots' max_seq; its buffers too are allocated and touched beforehand; median of --reps calls after one of warm-up);
  * what a resume costs without this feature: prefill_slot of the same length with the best exact options ("multi_extend_exact_mfma" or
    "multi_extend_mla_exact_mfma", "multi_extend_la_exact" with "multi_extend_la_exact_min" 2: those profiles/multi_extend_la_exact.txt was taken with).

    python tools/probes/slot_swap_cost.py [out.txt] [--reps 3] [--models qcn,v2l]
"""
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

import ctypes as C  # noqa: E402

import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
from krasis_amd._lib import check  # noqa: E402

PT = 64
CHUNKS = [1 << 20, 4 << 20, 16 << 20, 64 << 20, 256 << 20]


def wall(f):
    t0 = time.perf_counter(); r = f(); return time.perf_counter() - t0, r


class Images:
    """n image buffers of the size the library asks for, touched, and the C arrays of the two calls"""
    def __init__(self, st, slots, P):
        n = len(slots)
        self.st, self.n = st, n
        self.arrays = [np.zeros(st.slot_image_bytes(P), np.uint8) for _ in slots]
        self.slots = (C.c_int32 * n)(*slots); self.lens = (C.c_int32 * n)(*[P] * n); self.out = (C.c_int32 * n)()
        self.ptrs = (C.c_void_p * n)(*[a.ctypes.data for a in self.arrays]); self.sizes = (C.c_size_t * n)(*[a.size for a in self.arrays])

    def export(self):
        check(self.st._lib.kr_decode_slots_export(self.st._h, self.n, self.slots, self.lens, self.ptrs, self.sizes, 0))

    def import_(self):
        check(self.st._lib.kr_decode_slots_import(self.st._h, self.n, self.slots, self.ptrs, self.sizes, self.out))


def plain_copy(nbytes, reps):
    """one pinned hipMemcpy of nbytes in each direction -> (device to host s, host to device s), medians"""
    host = torch.empty(nbytes, dtype=torch.uint8).pin_memory(); dev = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    d2h, h2d = [], []
    for _ in range(reps + 1):
        torch.cuda.synchronize()
        d2h.append(wall(lambda: (host.copy_(dev), torch.cuda.synchronize()))[0])
        h2d.append(wall(lambda: (dev.copy_(host), torch.cuda.synchronize()))[0])
    return statistics.median(d2h[1:]), statistics.median(h2d[1:])


def old_buffers(layers, kv):
    """the host buffers of old_route, allocated and touched beforehand like the image buffers"""
    return [(kind, np.zeros(a(kv), np.uint8), np.zeros(b(kv), np.uint8)) for kind, a, b in layers]


def old_route(st, bufs, slots, P):
    """load_slot + get_decode_state of every layer, per slot: what leaves the device without this feature (the sampler does not)"""
    t0 = time.perf_counter()
    for s in slots:
        st.load_slot(s, P)
        for li, (kind, a, b) in enumerate(bufs):
            if kind == "la":
                st.get_decode_state(li, None, None, a, b)
            else:
                st.get_decode_state(li, a, b, None, None)
    return time.perf_counter() - t0


def measure(name, st, layers, opts, kv, reps, log, table):
    tokens = [(i * 31 + 7) % 1000 for i in range(4096)]
    prefill, bufs = {}, old_buffers(layers, kv)
    for o, v in opts:
        st.set_option(o, v)
    st.create_slots(1, kv)
    for P in (512, 4096):
        ts = [wall(lambda: st.prefill_slot(0, tokens[:P]))[0] for _ in range(3)]
        prefill[P] = statistics.median(ts[1:])
    log(f"{name}: prefill_slot with {', '.join(f'{o} {v}' for o, v in opts)}: " + ", ".join(f"{P} positions {t * 1e3:.1f} ms" for P, t in prefill.items()))
    for geo in ("pages of 64", "flat"):
        for n in (1, 16):
            for P in (512, 4096):
                paged = dict(page_tokens=PT, n_pages=n * ((P + PT - 1) // PT)) if geo != "flat" else {}
                st.create_slots(n, kv, **paged)
                st.reset_decode_state(kv); st.fill_state_synthetic(kv, seed=99)
                slots = list(range(n))
                for s in slots:
                    st.save_slot(s, P)
                nbytes = n * st.slot_image_bytes(P)
                log(f"{name}  {geo:<11}  {n:>2} slots x {P:>4} positions: {nbytes / 1e6:.1f} MB of images ({nbytes // n} bytes each)")
                im = Images(st, slots, P)
                first, best = None, {}
                for chunk in CHUNKS:
                    st.set_option("slot_swap_chunk_bytes", chunk)
                    te, ti = [], []
                    for _ in range(reps + 1):
                        te.append(wall(im.export)[0])
                        ti.append(wall(im.import_)[0])
                    if first is None:
                        first = [a.copy() for a in im.arrays]
                    assert all(np.array_equal(x, y) for x, y in zip(first, im.arrays)), "an image changed over a round trip"
                    e, i = statistics.median(te[1:]), statistics.median(ti[1:])
                    best[chunk] = e + i
                    log(f"    chunk {chunk >> 20:>3} MiB   export {e * 1e3:>9.3f} ms {nbytes / e / 1e9:>6.2f} GB/s   import {i * 1e3:>9.3f} ms {nbytes / i / 1e9:>6.2f} GB/s   "
                        f"sum {(e + i) * 1e3:>9.3f} ms")
                table.append(best)
                lo = min(best.values())
                pick = min(c for c, t in best.items() if t <= 1.05 * lo)
                log(f"    smallest chunk within 5 % of the best sum: {pick >> 20} MiB")
                del first, im
                d2h, h2d = plain_copy(nbytes, reps)
                log(f"    ceiling, one pinned copy   device to host {d2h * 1e3:>9.3f} ms {nbytes / d2h / 1e9:>6.2f} GB/s   host to device {h2d * 1e3:>9.3f} ms {nbytes / h2d / 1e9:>6.2f} GB/s")
                t_old = statistics.median([old_route(st, bufs, slots, P) for _ in range(reps + 1)][1:])
                log(f"    floor, load_slot + get_decode_state of every layer (no way back): {t_old * 1e3:>9.1f} ms")
                log(f"    resume without this feature, prefill_slot of {P} tokens per slot: {n * prefill[P] * 1e3:>9.1f} ms ({n} x {prefill[P] * 1e3:.1f})")
    st.set_option("slot_swap_chunk_bytes", 4 << 20)
    st.create_slots(0, 1)


def main():
    reps, models = 3, ["qcn", "v2l"]
    if "--reps" in sys.argv:
        i = sys.argv.index("--reps"); reps = int(sys.argv[i + 1]); del sys.argv[i:i + 2]
    if "--models" in sys.argv:
        i = sys.argv.index("--models"); models = sys.argv[i + 1].split(","); del sys.argv[i:i + 2]
    out_path = sys.argv[1] if len(sys.argv) > 1 else None
    kv = 4096 + 160
    lines, table = [], []

    def log(s):
        print(s, flush=True); lines.append(s)
        if out_path:      # as it goes: a run that is cut short leaves what it measured
            with open(out_path, "w") as f:
                f.write("\n".join(lines) + "\n")

    log("tools/probes/slot_swap_cost.py: one MI355X, exact mode, E4M3 caches, slots of %d positions; wall times, median of %d calls after one of warm-up" % (kv, reps))
    if "qcn" in models:
        q = bench.QCN
        eng, st, keep = bench.build_qcn(0, 0, 48, rope_len=kv, kv_fp8=True)
        conv, rec, row = (2 * q["nk"] * q["dk"] + q["nv"] * q["dv"]) * 16, q["nv"] * q["dk"] * q["dv"] * 4, q["nkv"] * q["hd"]
        layers = [("kv", lambda m: m * row, lambda m: m * row) if bench.is_gqa(l) else ("la", lambda m: conv, lambda m: rec) for l in range(48)]
        measure("QCN", st, layers, [("multi_extend_exact_mfma", 1), ("multi_extend_la_exact", 1), ("multi_extend_la_exact_min", 2)], kv, reps, log, table)
        del eng, st, keep
    if "v2l" in models:
        v = bench.V2L
        eng, st, keep = bench.build_v2lite(0, 0, v["layers"], rope_len=kv, kv_fp8=True)
        layers = [("kv", lambda m: m * v["klr"], lambda m: m * v["rd"])] * v["layers"]
        measure("V2-Lite", st, layers, [("multi_extend_mla_exact_mfma", 1)], kv, reps, log, table)
    # over the whole table: every configuration's sum, added up, and its ratio to that configuration's best; the default is the smallest chunk whose total is
    # within 5 % of the best total
    log("all configurations together, export + import:")
    total = {c: sum(b[c] for b in table) for c in CHUNKS}
    for c in CHUNKS:
        ratios = [b[c] / min(b.values()) for b in table]
        log(f"    chunk {c >> 20:>3} MiB   total {total[c] * 1e3:>9.1f} ms   against each configuration's best: geometric mean {np.exp(np.mean(np.log(ratios))):.3f}, worst {max(ratios):.3f}")
    log(f"    smallest chunk whose total is within 5 % of the best total: {min(c for c in CHUNKS if total[c] <= 1.05 * min(total.values())) >> 20} MiB")


if __name__ == "__main__":
    main()
