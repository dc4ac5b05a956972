"""Random call orders on paged and forked slots (docs/design/21-paged-slots.md, 22-slot-fork.md).  A seeded driver keeps, per slot, nothing but its token
history -- a slot's observable state is a function of that list -- and draws about 60 operations over the slot entry points: step_multi, extend_multi (on stores
without linear attention also from below the slot's length: a rewind, which forces copy-on-write), verify_multi + commit_multi, fork_slot, trim_slot, a
load_slot / save_slot round trip, generate_multi.  The pool is small enough to run out now and then: a call refused for the pool must leave every table row,
reference count and free count as they were.  After every operation the page tables are checked against the histories; at checkpoints one step over all live
slots is compared row by row with the single-sequence path (prefill(history), decode_step: logits bits and the state snapshot); at the end the successful
operations are replayed on flat slots of the same store and every id and logits array must be the same.  The paged path is never its own reference."""
import numpy as np
import pytest

from krasis_amd._lib import KrasisHipError
from tests import test_multi_mla_gpu as mla
from tests.test_multi_paged_gpu import Gqa, Mla, _slot_state

pytestmark = pytest.mark.gpu
U = np.uint32
N_SLOTS, MAX_SEQ, PT, N_PAGES, N_OPS, CHECK_EVERY = 6, 200, 32, 18, 60, 20
OPS = ("step", "extend", "verify", "fork", "trim", "save", "generate")
WEIGHTS = np.array([0.14, 0.28, 0.10, 0.20, 0.08, 0.10, 0.10])


class Driver:
    """draws the operations and runs them on paged slots of `st`; log = the successful ones with their arguments, out = what they returned.  The sizes are
    instance attributes and the operation table a class attribute, so that a subclass can drive other sizes and further operations
    (tests/test_multi_options_random_gpu.py)"""
    OPS, WEIGHTS = OPS, WEIGHTS

    def __init__(self, K, st, d, seed, rewind, check=True, n_slots=N_SLOTS, max_seq=MAX_SEQ, pt=PT, n_pages=N_PAGES, n_ops=N_OPS, check_every=CHECK_EVERY):
        self.K, self.st, self.d, self.rewind, self.check = K, st, d, rewind, check
        self.n_slots, self.max_seq, self.pt, self.n_pages, self.n_ops, self.check_every = n_slots, max_seq, pt, n_pages, n_ops, check_every
        self.rng = np.random.default_rng(seed)
        self.hist = [[] for _ in range(n_slots)]
        self.log, self.out, self.names = [], [], []
        self.refused = self.copies = self.checkpoints = 0

    # ---- the page tables against the histories
    def tables(self):
        return [self.st.slot_page_ids(s) for s in range(self.n_slots)], self.st.slot_pages()

    def shadow(self):
        rows, pages = self.tables()
        named = {}
        for s, (ids, refs) in enumerate(rows):
            need = (len(self.hist[s]) + self.pt - 1) // self.pt
            assert all(i >= 0 for i in ids[:need]), ("positions [0, len) are mapped", s, len(self.hist[s]), ids)
            assert pages["per_slot"][s] == sum(i >= 0 for i in ids), ("per_slot", s)
            for i in ids:
                if i >= 0:
                    assert i < self.n_pages
                    named[i] = named.get(i, 0) + 1
        for s, (ids, refs) in enumerate(rows):
            assert refs == [named.get(i, 0) if i >= 0 else 0 for i in ids], ("refs = the table entries naming the page", s, ids, refs)
        assert pages["free"] == self.n_pages - len(named), ("free = n_pages - the distinct pages named", pages["free"], sorted(named))
        return rows

    def count_copies(self, before, after):
        """a table entry that changed while its old page keeps another holder"""
        still = {i for ids, _ in after for i in ids if i >= 0}
        for (b, _), (a, _) in zip(before, after):
            self.copies += sum(1 for x, y in zip(b, a) if x >= 0 and y >= 0 and x != y and x in still)

    # ---- drawing
    def toks(self, n):
        return [int(x) for x in self.rng.integers(0, self.d["V"], n)]

    def subset(self, pool, hi):
        pool = list(pool)
        n = int(self.rng.integers(1, min(hi, len(pool)) + 1))
        return [int(x) for x in self.rng.permutation(pool)[:n]]

    def run_len(self, p):
        """the tokens of a run that enters at position p"""
        return int(self.rng.integers(1, min(70, self.max_seq - p) + 1))

    def draw(self):
        r, h = self.rng, self.hist
        room = [s for s in range(self.n_slots) if len(h[s]) < self.max_seq - 8]
        live = [s for s in range(self.n_slots) if h[s]]
        name = self.OPS[int(r.choice(len(self.OPS), p=self.WEIGHTS))]
        if name == "step" and room:
            sl = self.subset(room, 5)
            return ("step", sl, self.toks(len(sl)), [len(h[s]) for s in sl])
        if name == "extend" and room:
            sl = self.subset(room, 3)
            pos = [int(r.integers(0, len(h[s]) + 1)) if self.rewind and h[s] and r.random() < 0.4 else len(h[s]) for s in sl]
            return ("extend", sl, [self.toks(self.run_len(p)) for p in pos], pos)
        if name == "verify" and room:
            sl = self.subset(room, 3)
            return ("verify", sl, [self.toks(int(r.integers(2, 9))) for _ in sl], [len(h[s]) for s in sl], [float(r.random()) for _ in sl])
        if name == "fork" and live:
            src = int(r.choice(live))
            dsts = self.subset([s for s in range(self.n_slots) if s != src], 3)
            return ("fork", src, dsts, int(r.integers(0, len(h[src]) + 1)) if self.rewind and r.random() < 0.5 else len(h[src]))
        if name == "trim" and live:
            s = int(r.choice(live))      # with linear attention only what lies past the slot's length may go: the layers' state cannot be cut back
            return ("trim", s, int(r.integers(0, len(h[s]) + 1)) if self.rewind else len(h[s]))
        if name == "save" and live:
            s = int(r.choice(live))
            return ("save", s, s if r.random() < 0.5 else int(r.integers(0, self.n_slots)), len(h[s]))      # onto itself: every page it shares is written, so copied
        if name == "generate" and room:
            sl = self.subset(room, 3)
            return ("generate", sl, self.toks(len(sl)), [len(h[s]) for s in sl], int(r.integers(2, 7)))
        return self.draw_more(name, room, live)

    def draw_more(self, name, room, live):
        """an operation of a subclass's table (or one that cannot be drawn now: None, the driver draws again)"""
        return None

    # ---- running one operation on whatever slots `st` has now: -> what it returned, and the histories afterwards
    @staticmethod
    def run(st, op, hist):
        h = [list(x) for x in hist]
        name = op[0]
        if name == "step":
            _, sl, tk, pos = op
            ids, lg = st.step_multi(sl, tk, pos, logits=True)
            for s, t in zip(sl, tk):
                h[s].append(t)
            return (list(ids), lg.view(U).copy()), h
        if name == "extend":
            _, sl, runs, pos = op
            ids, lg = st.extend_multi(sl, runs, pos, logits=True)
            for s, run, p in zip(sl, runs, pos):
                h[s] = h[s][:p] + run
            return (list(ids), lg.view(U).copy()), h
        if name == "verify":
            _, sl, runs, pos, u = op
            ids, nm = st.verify_multi(sl, runs, pos)
            keep = [int(x * (m + 2)) for x, m in zip(u, nm)]      # 0 .. n_match + 1
            st.commit_multi(keep)
            for s, run, k in zip(sl, runs, keep):
                h[s] += run[:k]
            return ([g[:m + 1] for g, m in zip(ids, nm)], list(nm)), h
        if name == "fork":
            _, src, dsts, n = op
            st.fork_slot(src, dsts, n)
            for t in dsts:
                h[t] = h[src][:n]
            return None, h
        if name == "trim":
            _, s, n = op
            st.trim_slot(s, n)
            h[s] = h[s][:n]
            return None, h
        if name == "save":
            _, s, t, n = op
            st.load_slot(s, n)
            st.save_slot(t, n)
            h[t] = list(h[s])
            return None, h
        _, sl, firsts, pos, n = op
        T = st.generate_multi(sl, firsts, pos, n)
        for s, f, t in zip(sl, firsts, T):
            assert len(t) == n
            h[s] += [f] + t[:-1]
        return [list(t) for t in T], h

    def step(self, op):
        before = self.shadow() if self.check else self.tables()[0]
        try:
            out, hist = self.run(self.st, op, self.hist)
        except RuntimeError as e:      # KR_ERR_STATE: the pool cannot give what the call needs -- nothing ran and nothing changed
            assert not isinstance(e, KrasisHipError) and "page pool" in str(e), e
            assert self.tables()[0] == before, ("a refused call changed the tables", op)
            self.refused += 1
            self.names.append(op[0] + " (refused)")
            return False
        self.hist = hist
        self.log.append(op); self.out.append(out); self.names.append(op[0])
        after = self.shadow() if self.check else self.tables()[0]
        if op[0] != "fork":      # a fork swaps whole rows; everything else changes a mapped entry only by copy-on-write
            self.count_copies(before, after)
        return True

    def checkpoint(self):
        """one step over all live slots against the single-sequence path, row by row (unless the pool refuses it), then every live slot's stored state"""
        K, st, d = self.K, self.st, self.d
        sl = [s for s in range(self.n_slots) if 0 < len(self.hist[s]) < self.max_seq - 8]
        stepped = bool(sl) and self.step(("step", sl, self.toks(len(sl)), [len(self.hist[s]) for s in sl]))
        if not self.check:
            return
        self.checkpoints += 1
        for s in range(self.n_slots):
            n = len(self.hist[s])
            if not n:
                continue
            K.start(st, d, self.hist[s][:-1])
            st.decode_step(self.hist[s][-1], n - 1)
            if stepped and s in sl:
                ids, lg = self.out[-1]
                assert np.array_equal(st.read_logits().view(U), lg[sl.index(s)]) and st.last_token() == ids[sl.index(s)], ("checkpoint", s)
            want = K.snap(st, d, n)
            K.same(_slot_state(K, st, d, s, n), want)

    def drive(self):
        done = 0
        while done < self.n_ops:
            op = self.draw()
            if op is None:
                continue
            self.step(op)
            done += 1
            if done % self.check_every == 0:
                self.checkpoint()


MODELS = {
    "hybrid": (Gqa, dict(fp8=False, seed=3, hd=64, nh=4), False),
    "hybrid-e4m3": (Gqa, dict(fp8=True, seed=3, hd=64, nh=4), False),
    "gqa-only": (Gqa, dict(fp8=False, seed=5, kinds=["gqa", "gqa"]), True),
    "gqa-only-e4m3": (Gqa, dict(fp8=True, seed=5, kinds=["gqa", "gqa"]), True),
    "mla": (Mla, dict(fp8=False, **mla.CFGS[0]), True),
    "mla-klr256-e4m3": (Mla, dict(fp8=True, **mla.CFGS[2]), True),
}
SEEDS = (104, 106, 107)


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("model", list(MODELS))
def test_random_call_orders(model, seed):
    K, cfg, rewind = MODELS[model]
    st, keep, d = K.build(kv_max=MAX_SEQ + 8, **cfg)
    st.reset_decode_state(d["kv_max"])                            # the store's own caches in the element type chosen above: load_slot fills them
    st.create_slots(N_SLOTS, MAX_SEQ, page_tokens=PT, n_pages=N_PAGES)
    drv = Driver(K, st, d, seed, rewind)
    try:
        drv.drive()
        # what the sequence must contain to be worth its time: conditions on the drawn calls, met by the choice of pool size, weights and seeds
        n = len(drv.names)
        assert 1 <= drv.refused <= n // 4, ("refused calls", drv.refused, n)
        assert drv.copies >= 3, ("copy-on-write copies", drv.copies)
        assert drv.checkpoints == N_OPS // CHECK_EVERY
        # the same successful calls on flat slots: every id and logits array is the same
        st.create_slots(N_SLOTS, MAX_SEQ)
        hist = [[] for _ in range(N_SLOTS)]
        for k, (op, want) in enumerate(zip(drv.log, drv.out)):
            got, hist = Driver.run(st, op, hist)
            if op[0] in ("step", "extend"):
                assert got[0] == want[0] and np.array_equal(got[1], want[1]), ("flat replay", k, op[0])
            else:
                assert got == want, ("flat replay", k, op[0])
        assert hist == drv.hist
    except BaseException:
        print("model %s seed %d: refused %d, copies %d" % (model, seed, drv.refused, drv.copies))
        for k, name in enumerate(drv.names):
            print(k, name)
        for op in drv.log:
            print(op[0], [x if not isinstance(x, list) or len(str(x)) < 80 else "[%d ...]" % len(x) for x in op[1:]])
        raise
