"""The exact slot options together, and changed between calls on live slots (docs/design/37-multi-options-together.md).  Seven opt-in forms of the batched pass
promise "no bit changes" -- "multi_attn_exact_split", "multi_mla_exact_split", "multi_extend_exact_mfma", "multi_extend_mla_exact_mfma", "multi_extend_la_exact",
"pass_few_rows" and "gguf_exact_pass" / "gguf_exact_grouped" -- and each has a file of its own that holds it alone against the option-off call.  Here they run
together.

1. Random call orders (the driver of tests/test_multi_paged_random_gpu.py, subclassed): before every drawn operation an option set is drawn for the store and
   applied, after the call everything is off again; a verify draws a second set between verify_multi and commit_multi.  Sampled operations join the table
   (step_multi_sample, verify_multi_sample + commit_multi; every slot's sampler is set at its first use).  The slots start at lengths on both sides of position
   256 (the GQA split's score tile), 64 (the MLA split's) and the page edges.  Every reference computation runs with all options off: the checkpoints against
   the single-sequence path, the final states against prefill(history) + decode_step, the replay of the successful calls on flat slots.  A second flat replay
   runs every call under the option set it had.  The grow-only buffers of the pass (scores, matrix-core rows, tile tables, scratch, few-row images) are so
   reused by successive passes with different layouts.
2. One scripted scenario per model family on paged slots with a fork in it, run with every option off (the reference), with every applicable option on, and
   with each option left out in turn.

The library says which forms a pass took (multi_path_counts, a host-side test aid): a sequence must contain enough passes that took each form and enough that
did not, and a scripted run must show exactly the forms that were switched on.  Every assertion is on ids and u32 / stored-row bit patterns."""
import numpy as np
import pytest

from tests.test_multi_paged_gpu import Gqa, Mla, _slot_state
from tests.test_multi_paged_random_gpu import Driver

pytestmark = pytest.mark.gpu
U = np.uint32
N_SLOTS, MAX_SEQ, PT, N_OPS, CHECK_EVERY = 6, 320, 32, 60, 20
FILL = (0, 31, 120, 250, 255, 300)      # the slots' lengths before the first drawn call
P_ON = 0.6                              # the draw: each applicable option is on with this probability

# option -> the counter of the passes that took its form, the counter of the passes with a row of that kind
FORMS = {
    "multi_attn_exact_split": ("xs_split", "passes"), "multi_mla_exact_split": ("mla_xs_split", "passes"),
    "multi_extend_exact_mfma": ("gqa_xm", "runs"), "multi_extend_mla_exact_mfma": ("mla_xm", "runs"), "multi_extend_la_exact": ("lx", "runs"),
    "pass_few_rows": ("few", "passes"), "gguf_exact_grouped": ("gguf_grouped", "gguf_exact"),
}
BY_LAYER = {"gqa": ("multi_attn_exact_split", "multi_extend_exact_mfma"), "la": ("multi_extend_la_exact",),
            "mla": ("multi_mla_exact_split", "multi_extend_mla_exact_mfma")}
# value option -> (the option it belongs to, the library's default, what the draw takes it from, its value in the scripted scenario)
VALUES = {
    "multi_attn_exact_split_min": ("multi_attn_exact_split", 512, (1, 33, 257), 1),
    "multi_mla_exact_split_min": ("multi_mla_exact_split", 512, (1, 33, 257), 1),
    "multi_extend_la_exact_min": ("multi_extend_la_exact", 8, (2, 8, 17), 2),
    "pass_few_rows_max": ("pass_few_rows", 16, (1, 5, 16), 16),
    "pass_few_rows_group": ("pass_few_rows", 0, (0, 3, 16), 0),
}


class Options:
    """the options applicable to a store of these layer kinds: flags (0 / 1; on a GGUF store "gguf_exact_grouped" among them, default 1) and their values"""

    def __init__(self, layers, gguf=False):
        self.flags = tuple(f for kind in layers for f in BY_LAYER[kind]) + ("pass_few_rows",) + (("gguf_exact_grouped",) if gguf else ())
        self.values = {v: spec for v, spec in VALUES.items() if spec[0] in self.flags}
        self.off = {f: 0 for f in self.flags}
        self.off.update({v: spec[1] for v, spec in self.values.items()})
        if gguf:
            self.off["gguf_exact_grouped"] = 1

    def draw(self, rng, p_on):
        s = {f: int(rng.random() < p_on) for f in self.flags}
        s.update({v: int(rng.choice(spec[2])) for v, spec in self.values.items()})
        return s

    def scripted(self, on):
        s = dict(self.off)
        s.update({f: int(f in on) for f in self.flags})
        s.update({v: spec[3] for v, spec in self.values.items()})
        return s

    @staticmethod
    def apply(st, s):
        for name, value in s.items():
            st.set_option(name, value)

    @staticmethod
    def show(s):
        return " ".join("%s=%d" % (k.replace("multi_", "").replace("extend_", "x_"), v) for k, v in s.items())


def run_op(st, op, hist, sets, off):
    """one operation under its option sets -- sets[0]; a verify commits under sets[1] -- and every option off again afterwards, also where the call is refused"""
    name = op[0]
    try:
        Options.apply(st, sets[0])
        if name in ("verify", "verify_s"):
            _, sl, runs, pos, u = op
            ids, nm = (st.verify_multi_sample if name == "verify_s" else st.verify_multi)(sl, runs, pos)
            keep = [int(x * (m + 2)) for x, m in zip(u, nm)]      # 0 .. n_match + 1
            Options.apply(st, sets[1])
            st.commit_multi(keep)
            h = [list(x) for x in hist]
            for s, run, k in zip(sl, runs, keep):
                h[s] += run[:k]
            return ([g[:m + 1] for g, m in zip(ids, nm)], list(nm)), h
        if name == "step_s":
            _, sl, tk, pos = op
            ids, lg = st.step_multi_sample(sl, tk, pos, logits=True)
            h = [list(x) for x in hist]
            for s, t in zip(sl, tk):
                h[s].append(t)
            return (list(ids), lg.view(U).copy()), h
        if name == "sampler":
            st.set_slot_sampler(*op[1:])
            return None, [list(x) for x in hist]
        return Driver.run(st, op, hist)
    finally:
        Options.apply(st, off)


def same_out(got, want, where):
    if isinstance(want, tuple) and len(want) == 2 and isinstance(want[1], np.ndarray):      # (ids, logits bits)
        assert got[0] == want[0] and np.array_equal(got[1], want[1]), where
    else:
        assert got == want, where


# per slot: temperature, top_k, top_p, presence penalty -- greedy, sampled, and greedy under a penalty
SAMPLERS = [(0.0, 0, 1.0, 0.0), (0.7, 40, 0.95, 0.3), (0.9, 20, 0.9, 0.0), (1.1, 64, 1.0, 0.5), (0.8, 8, 0.8, 0.2), (0.0, 0, 1.0, 0.5)]


class OptionDriver(Driver):
    """the parent's operations and the sampled ones, each under an option set of its own; sets / deltas = per successful operation the sets it ran under and
    what it added to multi_path_counts"""
    OPS = Driver.OPS + ("step_s", "verify_s", "extend_few")
    WEIGHTS = np.array([0.10, 0.16, 0.09, 0.13, 0.06, 0.06, 0.06, 0.05, 0.05, 0.24])

    def __init__(self, K, st, d, seed, rewind, options, n_pages, p_on, **kw):
        super().__init__(K, st, d, seed, rewind, n_slots=N_SLOTS, max_seq=MAX_SEQ, pt=PT, n_pages=n_pages, n_ops=N_OPS, check_every=CHECK_EVERY, **kw)
        self.options, self.p_on = options, p_on
        self.orng = np.random.default_rng(seed + 1000)      # the option sets have a stream of their own: the drawn calls do not depend on p_on
        self.sets, self.deltas, self.cur = [], [], None
        self.drawn = (0, 0)      # where the drawn calls begin in deltas and in names: the conditions are about them, not about the set-up of start()

    def run_len(self, p):
        """a quarter unit rows, a quarter short runs, the rest any length up to 70"""
        r, top = self.rng, min(70, self.max_seq - p)
        kind = r.random()
        return 1 if kind < 0.25 else int(r.integers(2, min(8, top) + 1)) if kind < 0.5 and top >= 2 else int(r.integers(1, top + 1))

    def draw_more(self, name, room, live):
        r, h = self.rng, self.hist
        if name == "step_s" and room:
            sl = self.subset(room, 5)
            return ("step_s", sl, self.toks(len(sl)), [len(h[s]) for s in sl])
        if name == "verify_s" and room:
            sl = self.subset(room, 3)
            return ("verify_s", sl, [self.toks(int(r.integers(2, 9))) for _ in sl], [len(h[s]) for s in sl], [float(r.random()) for _ in sl])
        if name == "extend_few" and room:
            # a decode row (two, or a second short run) beside a short chunk, at most 5 or at most 9 token rows in all: an extend_multi small enough for the
            # few-row form that holds a run of two or more tokens AND a unit row, so that the few-row kernels, a split -- which under a matrix-core run form
            # is launched for the unit rows only -- and a matrix-core or staged pass can meet
            sl = [int(x) for x in r.permutation(list(room))[:min(len(room), int(r.integers(2, 4)))]]
            pos = [int(r.integers(0, len(h[s]) + 1)) if self.rewind and h[s] and r.random() < 0.4 else len(h[s]) for s in sl]
            tiny = r.random() < 0.5
            lens = ([int(r.integers(2, 4)), 1] + [1 if tiny else int(r.integers(1, 6)) for _ in sl[2:]])[:len(sl)]
            return ("extend", sl, [self.toks(min(n, self.max_seq - p)) for n, p in zip(lens, pos)], pos)
        return None

    def run(self, st, op, hist):
        return run_op(st, op, hist, self.cur, self.options.off)

    def step(self, op, sets=None):
        self.cur = sets or (self.options.draw(self.orng, self.p_on), self.options.draw(self.orng, self.p_on))
        before = self.st.multi_path_counts()
        ok = super().step(op)
        after = self.st.multi_path_counts()
        delta = {k: after[k] - before[k] for k in after}
        if ok:
            self.sets.append(self.cur); self.deltas.append(delta)
        else:
            assert delta["passes"] == 0, ("a refused call ran a pass", op[0], delta)
        self.names[-1] += "   " + Options.show(self.cur[0]) + ("   commit: " + Options.show(self.cur[1]) if op[0].startswith("verify") else "")
        assert all(v == 0 for k, v in delta.items() if k in ("fd", "mla_fd", "gqa_flash", "mla_flash", "lc")), delta      # no tolerance form anywhere
        return ok

    def start(self):
        """every slot's sampler at its first use, then the prompts by prefill_slot's one call (an extend of one run), all options off"""
        off = (self.options.off, self.options.off)
        for s, (t, k, p, pen) in enumerate(SAMPLERS[:self.n_slots]):
            assert self.step(("sampler", s, self.toks(1)[0], t, k, p, pen, 100 + s), off)
        for s, n in enumerate(FILL):
            if n:
                assert self.step(("extend", [s], [self.toks(n)], [0]), off), ("the pool holds the prompts", s, n)
        self.drawn = (len(self.deltas), len(self.names))

    def reference_states(self):
        """every live slot's state by the single-sequence path, options off: prefill(history[:-1]), decode_step(history[-1])"""
        K, st, d, want = self.K, self.st, self.d, {}
        for s in range(self.n_slots):
            n = len(self.hist[s])
            if n:
                K.start(st, d, self.hist[s][:-1])
                st.decode_step(self.hist[s][-1], n - 1)
                want[s] = K.snap(st, d, n)
        return want

    def conditions(self):
        """what the drawn calls (checkpoints among them, the set-up of start() not) must contain to be worth their time, from multi_path_counts over the paged
        run: -> (figures, the conditions that are not met)"""
        deltas, log, sets = self.deltas[self.drawn[0]:], self.log[self.drawn[0]:], self.sets[self.drawn[0]:]
        total = {k: sum(dl[k] for dl in deltas) for k in self.deltas[0]}
        fig, bad = {}, []
        for f in self.options.flags:
            form, kind = FORMS[f]
            fig[f] = (total[form], total[kind] - total[form])
            if total[form] < 5:
                bad.append("%s: %d passes took its form (at least 5)" % (f, total[form]))
            if total[kind] - total[form] < 5:
                bad.append("%s: %d passes with a row of its kind did not take its form (at least 5)" % (f, total[kind] - total[form]))
        fig["three forms"] = sum(1 for dl in deltas if dl["passes"] == 1 and sum(dl[FORMS[f][0]] > 0 for f in self.options.flags) >= 3)
        if fig["three forms"] < 3:
            bad.append("%d passes took three or more option forms at once (at least 3)" % fig["three forms"])
        fig["verify under two sets"] = sum(1 for op, (a, b) in zip(log, sets) if op[0].startswith("verify") and a != b)
        if fig["verify under two sets"] < 2:
            bad.append("%d verify operations committed under another set than they verified under (at least 2)" % fig["verify under two sets"])
        fig["passes"], fig["few"], fig["verify"] = total["passes"], total["few"], total["verify"]
        return fig, bad


def replay(drv, st, with_sets, want_states, want_samplers):
    """the successful calls on flat slots -- every option off, or each call under the sets it had: ids, logits, n_match, tokens, sampler and slot states"""
    K, d, off = drv.K, drv.d, drv.options.off
    tag = "flat replay under the calls' option sets" if with_sets else "flat replay, options off"
    st.create_slots(drv.n_slots, drv.max_seq)
    hist = [[] for _ in range(drv.n_slots)]
    for k, (op, want, sets) in enumerate(zip(drv.log, drv.out, drv.sets)):
        got, hist = run_op(st, op, hist, sets if with_sets else (off, off), off)
        same_out(got, want, (tag, k, op[0]))
    assert hist == drv.hist
    for s, (seen, state) in enumerate(want_samplers):
        got_seen, got_state = st.slot_sampler_state(s)
        assert np.array_equal(got_seen, seen) and got_state == state, (tag, "sampler state", s)
    for s, want in want_states.items():
        K.same(_slot_state(K, st, d, s, len(hist[s])), want)


MODELS = {      # name -> (helpers, build arguments, rewinds, layer kinds, pages of the pool)
    "hybrid": (Gqa, dict(fp8=False, seed=3, hd=64, nh=4), False, ("gqa", "la"), 38),
    "hybrid-e4m3": (Gqa, dict(fp8=True, seed=3, hd=64, nh=4), False, ("gqa", "la"), 38),
    "gqa-only": (Gqa, dict(fp8=False, seed=5, kinds=["gqa", "gqa"]), True, ("gqa",), 32),
    "mla": (Mla, dict(fp8=False), True, ("mla",), 32),
    "mla-klr256-e4m3": (Mla, dict(fp8=True, klr=256, nh=4, seed=4), True, ("mla",), 32),
    "hybrid-gguf": (Gqa, dict(fp8=False, seed=11, dims=(256, 512, 8, 3, 256, 128), gguf=True), False, ("gqa", "la"), 38),
}
# seeds whose drawn calls meet the conditions asserted below (found by running seeds 201 .. 400: 14 of them do on the hybrid stores, 33 on the GGUF store, 9 on
# the stores with three options, where all three must be on in a pass of at most 16 rows that holds a run and a unit row)
SEEDS = {"hybrid": (238, 245), "hybrid-e4m3": (238, 245), "gqa-only": (213, 219), "mla": (213, 219), "mla-klr256-e4m3": (213, 219), "hybrid-gguf": (238, 245)}


def _build(model):
    K, cfg, rewind, layers, n_pages = MODELS[model]
    st, keep, d = K.build(kv_max=MAX_SEQ + 8, **cfg)
    gguf = bool(cfg.get("gguf"))
    if gguf:
        st.set_option("gguf_exact_pass", 1)      # on in the reference too: without it the store refuses slots, speculation and an exact prompt pass
    st.reset_decode_state(d["kv_max"])
    return K, st, keep, d, rewind, Options(layers, gguf), n_pages


@pytest.mark.parametrize("model,seed", [(m, s) for m in MODELS for s in SEEDS[m]])
def test_random_call_orders_under_random_option_sets(model, seed):
    K, st, keep, d, rewind, options, n_pages = _build(model)
    st.create_slots(N_SLOTS, MAX_SEQ, page_tokens=PT, n_pages=n_pages)
    st.multi_path_counts(reset=True)
    drv = OptionDriver(K, st, d, seed, rewind, options, n_pages, P_ON)
    fig = bad = None
    try:
        drv.start()
        drv.drive()
        fig, bad = drv.conditions()
        n = len(drv.names) - drv.drawn[1]      # the drawn calls and the checkpoints' steps, as in the parent test
        assert 1 <= drv.refused <= n // 4, ("refused calls", drv.refused, n)
        assert drv.copies >= 3, ("copy-on-write copies", drv.copies)
        assert drv.checkpoints == N_OPS // CHECK_EVERY
        # every live slot's final state against the single-sequence path, and the samplers as they stand
        want_states = drv.reference_states()
        for s, want in want_states.items():
            K.same(_slot_state(K, st, d, s, len(drv.hist[s])), want)
        want_samplers = [st.slot_sampler_state(s) for s in range(N_SLOTS)]
        replay(drv, st, False, want_states, want_samplers)
        replay(drv, st, True, want_states, want_samplers)
        print("model %s seed %d: %s" % (model, seed, fig))
        assert not bad, bad      # conditions on the drawn calls (choice of weights, pool and seeds), asserted last so that a sequence that misses them shows whether anything else fails
    except BaseException:
        print("model %s seed %d: refused %d, copies %d, %s, not met: %s" % (model, seed, drv.refused, drv.copies, fig, bad))
        for k, name in enumerate(drv.names):
            print(k, name)
        for op in drv.log:
            print(op[0], [x if not isinstance(x, list) or len(str(x)) < 80 else "[%d ...]" % len(x) for x in op[1:]])
        raise


# ---- one scripted scenario: all options off, all on, each one left out ---------------------------------------------------------------------------------------
def _scenario(K, st, d):
    """paged slots with a fork; everything the calls returned, the histories, the final slot states and sampler states"""
    rng = np.random.default_rng(77)
    T = lambda n: [int(x) for x in rng.integers(0, d["V"], n)]
    st.create_slots(6, MAX_SEQ, page_tokens=PT, n_pages=44)
    h, out = [[] for _ in range(6)], []
    at = lambda sl: [len(h[s]) for s in sl]

    def extend(sl, runs):
        ids, lg = st.extend_multi(sl, runs, at(sl), logits=True)
        for s, run in zip(sl, runs):
            h[s] += run
        out.append((list(ids), lg.view(U).copy()))

    def verify(sl, want):
        """the first draft token is the greedy one (learnt from a pass that is dropped), so n_match >= 1 and a commit can be partial: keep <= want"""
        firsts, pos = T(len(sl)), at(sl)
        g, nm = st.verify_multi(sl, [[f] + T(4) for f in firsts], pos)
        st.commit_multi([0] * len(sl))
        out.append(([row[:m + 1] for row, m in zip(g, nm)], list(nm)))
        runs = [[f, row[0]] + T(3) for f, row in zip(firsts, g)]
        g, nm = st.verify_multi(sl, runs, pos)
        assert all(m >= 1 for m in nm), nm
        keep = [min(m + 1, w) for m, w in zip(nm, want)]
        st.commit_multi(keep)
        for s, run, k in zip(sl, runs, keep):
            h[s] += run[:k]
        out.append(([row[:m + 1] for row, m in zip(g, nm)], list(nm)))

    def generated(sl, firsts, toks, n):
        for s, f, t in zip(sl, firsts, toks):
            assert len(t) == n
            h[s] += [f] + t[:-1]
        out.append([list(t) for t in toks])

    extend([0], [T(200)]); extend([1], [T(100)]); extend([2], [T(31)])
    st.fork_slot(0, [3], 200); h[3] = list(h[0])                        # six whole pages shared, the boundary page copied
    extend([0, 1, 2, 3, 4], [T(1), T(2), T(17), T(70), T(1)])           # unit rows at positions 200 and 0; the run of 70 crosses position 256 on the forked slot
    extend([0], [T(54)])
    for p in (255, 256, 257):
        assert len(h[0]) == p
        sl, tk = [0, 1, 4], T(3)
        ids, lg = st.step_multi(sl, tk, at(sl), logits=True)
        for s, t in zip(sl, tk):
            h[s].append(t)
        out.append((list(ids), lg.view(U).copy()))
    verify([0, 2, 3], [2, 1, 0])                                          # 15 rows: the few-row form
    verify([0, 1, 2, 3], [1, 2, 0, 2])                                    # 20 rows: not
    sl, f = [1, 4], T(2)
    generated(sl, f, st.generate_multi(sl, f, at(sl), 6), 6)
    sl, f = [1, 2], T(2)
    generated(sl, f, st.generate_multi_lookup(sl, f, at(sl), 8, contexts=[list(h[1]), list(h[2])]), 8)
    out.append(dict(st.last_multi_lookup_stats))
    sl, f = [1, 4], T(2)
    generated(sl, f, st.generate_multi_lookup_sample(sl, f, at(sl), 8, contexts=[list(h[1]), list(h[4])], temperature=[0.8, 0.0], top_k=[40, 20],
                                                     top_p=[0.95, 1.0], presence_penalty=[0.3, 0.5], rng_seeds=[11, 12]), 8)
    out.append(dict(st.last_multi_lookup_stats))
    samplers = [st.slot_sampler_state(s) for s in range(6)]
    states = {s: _slot_state(K, st, d, s, len(h[s])) for s in range(6) if h[s]}
    return out, h, states, samplers


@pytest.mark.parametrize("model", ["hybrid-e4m3", "mla-klr256-e4m3"])
def test_scripted_scenario_all_options_on_and_leave_one_out(model):
    K, st, keep, d, rewind, options, _ = _build(model)
    flags = options.flags
    legs = [("all off", ())] + [("all on", flags)] + [("all but " + f, tuple(g for g in flags if g != f)) for f in flags]
    ref = None
    for tag, on in legs:
        st.multi_path_counts(reset=True)
        Options.apply(st, options.scripted(on))
        try:
            got = _scenario(K, st, d)
        finally:
            Options.apply(st, options.off)
        counts = st.multi_path_counts()
        took = {f for f in flags if counts[FORMS[f][0]] > 0}
        assert took == set(on), (tag, "the forms the passes took", sorted(took), counts)
        assert counts["passes"] >= 20 and counts["verify"] >= 4 and 0 < counts["runs"] < counts["passes"], (tag, counts)
        if "pass_few_rows" in on:
            assert 0 < counts["few"] < counts["passes"], (tag, counts)      # steps and the 15-row verify took the form, the prompts and the 20-row verify did not
        if ref is None:
            ref = got
            for s, want in ref[2].items():      # the reference run itself against the single-sequence path
                K.start(st, d, ref[1][s][:-1])
                st.decode_step(ref[1][s][-1], len(ref[1][s]) - 1)
                K.same(want, K.snap(st, d, len(ref[1][s])))
            continue
        assert len(got[0]) == len(ref[0])
        for k, (a, b) in enumerate(zip(got[0], ref[0])):
            same_out(a, b, (tag, "call", k))
        assert got[1] == ref[1], (tag, "histories")
        assert sorted(got[2]) == sorted(ref[2])
        for s in ref[2]:
            K.same(got[2][s], ref[2][s])
        for s, ((seen, state), (rseen, rstate)) in enumerate(zip(got[3], ref[3])):
            assert np.array_equal(seen, rseen) and state == rstate, (tag, "sampler state", s)
