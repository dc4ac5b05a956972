"""MLA layers in the exact batched multi-sequence decode (docs/design/15-multi-mla.md): every row of a multi-sequence step over a store whose
layers are MLA is BIT-IDENTICAL to kr_decode_step on that sequence alone -- logits, greedy id, the compressed-KV row [klr] and the rope-key row
[rd] it appends -- whatever rows share the step, in whatever order, at whatever positions, with FP16 or E4M3 latent caches, the direct or the
LoRA query path, kv_lora_rank 512 or 256.  The reference everywhere is the single-sequence path (decode_step / generate_batch), which
tests/test_mla_gpu.py holds to the CPU oracle bit for bit; the batched step is never compared with itself."""
import numpy as np
import pytest

from tests.test_mla_gpu import build

pytestmark = pytest.mark.gpu
F = np.float32
U = np.uint32

CFGS = [dict(), dict(lora=True, seed=2), dict(klr=256, nh=3, seed=4)]


def _build(fp8=False, **cfg):
    st, eng, orc, keep, d = build(**cfg)
    d["fp8"] = fp8
    if fp8:
        st.set_kv_dtype(True)
    return st, eng, keep, d


def _prompt(rng, d, n):
    return [int(x) for x in rng.integers(0, d["V"], n)]


def _start(st, d, prompt):
    """the store's own sequence = prompt (build leaves random caches: zero state first, then the prompt pass)"""
    st.reset_decode_state(d["kv_max"])
    if prompt:
        st.prefill(prompt, 0)


def _snap(st, d, pos):
    """rows [0, pos) of the latent and the rope-key cache of every layer, as stored (uint16: FP16, uint8: E4M3)"""
    t = np.uint8 if d["fp8"] else np.uint16
    out = []
    for li in range(d["nL"]):
        ck = np.empty((d["kv_max"], d["klr"]), t); kp = np.empty((d["kv_max"], d["rd"]), t)
        st.get_decode_state(li, ck, kp, None, None)
        out.append((ck[:pos].copy(), kp[:pos].copy()))
    return out


def _same(got, want):
    assert len(got) == len(want)
    for li, ((ck, kp), (rck, rkp)) in enumerate(zip(got, want)):
        assert np.array_equal(ck, rck), ("latent rows", li)
        assert np.array_equal(kp, rkp), ("rope-key rows", li)


def _reference(st, d, prompt, first, n_steps):
    """decode_step alone: per step (logits bits, greedy id); then the caches after the steps"""
    _start(st, d, prompt)
    out, tok, pos = [], first, len(prompt)
    for _ in range(n_steps):
        st.decode_step(tok, pos)
        out.append((st.read_logits().view(U).copy(), st.last_token()))
        tok = out[-1][1]; pos += 1
    return out, _snap(st, d, pos)


def _fill_slots(st, d, prompts, slot_lists):
    for p, slots in zip(prompts, slot_lists):
        _start(st, d, p)
        for s in slots:
            st.save_slot(s, len(p))


def _steps_against_refs(st, d, refs, slots, firsts, pos, n_steps):
    toks, pos = list(firsts), list(pos)
    for k in range(n_steps):
        ids, lg = st.step_multi(slots, toks, pos, logits=True)
        for i, (ref, _) in enumerate(refs):
            assert np.array_equal(lg[i].view(U), ref[k][0]), ("logits", k, i)
            assert ids[i] == ref[k][1], ("id", k, i)
        toks = ids; pos = [p + 1 for p in pos]
    return toks, pos


@pytest.mark.parametrize("fp8", [False, True])
@pytest.mark.parametrize("cfg", CFGS)
def test_step_multi_equals_decode_step_alone(cfg, fp8):
    st, eng, keep, d = _build(fp8, kv_max=64, **cfg)
    rng = np.random.default_rng(5)
    prompts = [_prompt(rng, d, n) for n in (1, 40, 7, 23, 12)] + [[]]      # the last slot starts at zero state, position 0
    firsts = [int(x) for x in rng.integers(0, d["V"], len(prompts))]
    refs = [_reference(st, d, p, f, 5) for p, f in zip(prompts, firsts)]
    st.create_slots(len(prompts) + 2, 60)
    slots = [3, 0, 6, 2, 5, 1]                                              # slot numbers need not follow the rows
    _fill_slots(st, d, prompts, [[s] for s in slots])
    toks, pos = _steps_against_refs(st, d, refs, slots, firsts, [len(p) for p in prompts], 4)
    for i, (ref, _) in enumerate(refs):
        ref_after4 = _reference(st, d, prompts[i], firsts[i], 4)[1]
        st.reset_decode_state(d["kv_max"])
        st.load_slot(slots[i], pos[i])
        _same(_snap(st, d, pos[i]), ref_after4)
        st.decode_step(toks[i], pos[i])                                     # the store continues the sequence identically
        assert np.array_equal(st.read_logits().view(U), ref[4][0]) and st.last_token() == ref[4][1], i


def test_batch_sizes_and_row_order():
    """B = 1, 31, 32, 33, 64 and the 64 rows permuted: crosses the 32-row switch of the absorption, w_vc and router forms"""
    st, eng, keep, d = _build(kv_max=48)
    rng = np.random.default_rng(9)
    n_seq = 64
    prompts = [_prompt(rng, d, int(rng.integers(1, 9))) for _ in range(n_seq)]
    firsts = [int(x) for x in rng.integers(0, d["V"], n_seq)]
    refs = [_reference(st, d, p, f, 1)[0][0] for p, f in zip(prompts, firsts)]
    batches = [1, 31, 32, 33, 64]
    perm = [int(x) for x in rng.permutation(64)]
    groups, base = [], 0
    for B in batches:
        groups.append((list(range(B)), list(range(base, base + B)))); base += B
    groups.append((perm, list(range(base, base + 64)))); base += 64        # the 64 rows again, permuted
    st.create_slots(base, 48)
    per_seq = [[] for _ in range(n_seq)]
    for seqs, slots in groups:
        for q, s in zip(seqs, slots):
            per_seq[q].append(s)
    _fill_slots(st, d, prompts, per_seq)
    for seqs, slots in groups:
        ids, lg = st.step_multi(slots, [firsts[q] for q in seqs], [len(prompts[q]) for q in seqs], logits=True)
        for r, q in enumerate(seqs):
            assert np.array_equal(lg[r].view(U), refs[q][0]), (len(seqs), r, q)
            assert ids[r] == refs[q][1], (len(seqs), r, q)


@pytest.mark.parametrize("kv_max,lens,cap", [(600, (40, 300, 590), 640), (8600, (300, 4100, 8400), 8500)])
@pytest.mark.parametrize("cfg,fp8", [(dict(nh=11), False), (dict(klr=256, seed=4), True), (dict(seed=6), True)])
def test_long_caches(cfg, fp8, kv_max, lens, cap):
    """the exact decode step picks its attention form from the store's kv_max_seq (score row in LDS up to 512, head-shared scores launch above,
    streamed score row for the longest); the batched kernel has one form.  Short, middle and long rows in one step, a ragged head group (nh 11),
    slot capacity different from the store's kv_max_seq."""
    st, eng, keep, d = _build(fp8, kv_max=kv_max, **cfg)
    rng = np.random.default_rng(kv_max)
    prompts = [_prompt(rng, d, n) for n in lens]
    firsts = [int(x) for x in rng.integers(0, d["V"], 3)]
    refs = [_reference(st, d, p, f, 2) for p, f in zip(prompts, firsts)]
    st.create_slots(3, cap)
    slots = [2, 0, 1]
    _fill_slots(st, d, prompts, [[s] for s in slots])
    toks, pos = _steps_against_refs(st, d, refs, slots, firsts, [len(p) for p in prompts], 2)
    for i, (_, snap) in enumerate(refs):
        st.reset_decode_state(kv_max)
        st.load_slot(slots[i], pos[i])
        _same(_snap(st, d, pos[i]), snap)


def test_generate_multi_equals_generate_greedy():
    st, eng, keep, d = _build(kv_max=64)
    rng = np.random.default_rng(13)
    prompts = [_prompt(rng, d, n) for n in (5, 17, 2, 30)]
    firsts = [int(x) for x in rng.integers(0, d["V"], 4)]
    max_tokens = 9
    free = []
    for p, f in zip(prompts, firsts):
        _start(st, d, p); free.append(st.generate_batch(f, len(p), max_tokens))
    stop_ids = [free[0][2], free[2][5]]                                     # rows end at different steps; rows without them reach max_tokens
    ref_toks, ref_snaps = [], []
    for p, f in zip(prompts, firsts):
        _start(st, d, p)
        T = st.generate_batch(f, len(p), max_tokens, stop_ids=stop_ids)
        ref_toks.append(T); ref_snaps.append(_snap(st, d, len(p) + len(T)))
    assert len({len(T) for T in ref_toks}) > 1 and max(len(T) for T in ref_toks) == max_tokens
    st.create_slots(4, 64)
    slots = [1, 3, 0, 2]
    _fill_slots(st, d, prompts, [[s] for s in slots])
    out = st.generate_multi(slots, firsts, [len(p) for p in prompts], max_tokens, stop_ids)
    assert out == ref_toks
    for i, p in enumerate(prompts):
        st.reset_decode_state(d["kv_max"])
        st.load_slot(slots[i], len(p) + len(out[i]))
        _same(_snap(st, d, len(p) + len(out[i])), ref_snaps[i])


def test_generate_multi_sampled_equals_generate_batch():
    """the server defaults (temperature 0.6, top_k 50, top_p 0.95) with fixed seeds, plus one penalised-greedy row"""
    st, eng, keep, d = _build(kv_max=64)
    rng = np.random.default_rng(21)
    prompts = [_prompt(rng, d, n) for n in (5, 17, 2, 30)]
    firsts = [int(x) for x in rng.integers(0, d["V"], len(prompts))]
    params = [(0.6, 50, 0.95, 0.0), (0.6, 50, 0.95, 0.0), (0.0, 0, 1.0, 1.5), (0.6, 50, 0.95, 0.0)]
    seeds = [0x1234567, 0x9E3779B9, 77, 5]
    max_tokens = 9
    ref_toks, ref_snaps = [], []
    for i, p in enumerate(prompts):
        _start(st, d, p)
        T, K, P, PEN = params[i]
        out = st.generate_batch(firsts[i], len(p), max_tokens, T, K, P, (), PEN, rng_seed=seeds[i])
        ref_toks.append(out); ref_snaps.append(_snap(st, d, len(p) + len(out)))
    slots = [1, 3, 0, 2]
    st.create_slots(4, 64)
    _fill_slots(st, d, prompts, [[s] for s in slots])
    out = st.generate_multi(slots, firsts, [len(p) for p in prompts], max_tokens, (),
                            temperature=[p[0] for p in params], top_k=[p[1] for p in params], top_p=[p[2] for p in params],
                            presence_penalty=[p[3] for p in params], rng_seeds=seeds)
    assert out == ref_toks
    for i, p in enumerate(prompts):
        st.reset_decode_state(d["kv_max"])
        st.load_slot(slots[i], len(p) + len(out[i]))
        _same(_snap(st, d, len(p) + len(out[i])), ref_snaps[i])


@pytest.mark.parametrize("graph", [True, False])
def test_steps_leave_the_store_sequence_alone(graph):
    st, eng, keep, d = _build(kv_max=48)
    st.set_use_graph(graph)
    rng = np.random.default_rng(17)
    prompt = _prompt(rng, d, 6)
    toks = _prompt(rng, d, 5)
    ref, _ = _reference(st, d, prompt, toks[0], 5)
    st.create_slots(3, 48)
    _fill_slots(st, d, [_prompt(rng, d, 3), _prompt(rng, d, 9)], [[0], [2]])
    _start(st, d, prompt)
    tok, pos, mpos = toks[0], len(prompt), [3, 9]
    for k in range(5):
        st.decode_step(tok, pos)
        ids = st.step_multi([2, 0], [toks[k], toks[-1 - k]], [mpos[1], mpos[0]])
        assert len(ids) == 2
        mpos = [p + 1 for p in mpos]
        assert np.array_equal(st.read_logits().view(U), ref[k][0]) and st.last_token() == ref[k][1], k
        tok = st.last_token(); pos += 1


@pytest.mark.parametrize("fp8", [False, True])
def test_save_load_round_trip(fp8):
    st, eng, keep, d = _build(fp8, kv_max=40)
    st.fill_state_synthetic(d["kv_max"], seed=3)
    want = _snap(st, d, 29)
    esz = 1 if fp8 else 2
    assert st.create_slots(2, 36) == 2 * 36 * (d["klr"] + d["rd"]) * esz * d["nL"]      # bytes_out counts both halves of every MLA layer
    st.save_slot(1, 29)
    st.reset_decode_state(d["kv_max"])
    st.load_slot(1, 29)
    _same(_snap(st, d, 29), want)


def test_refusals_change_nothing():
    st, eng, keep, d = _build(kv_max=32)
    with pytest.raises(Exception):
        st.step_multi([0], [1], [0])                                       # no slots yet
    st.create_slots(3, 24)
    st.fill_state_synthetic(d["kv_max"], seed=5)
    st.save_slot(1, 20)
    want = _snap(st, d, 20)

    def unchanged():
        st.reset_decode_state(d["kv_max"]); st.load_slot(1, 20)
        _same(_snap(st, d, 20), want)

    V = d["V"]
    bad_steps = [([1, 1], [2, 3], [20, 20]),      # a slot named twice
                 ([3], [2], [20]), ([-1], [2], [20]),   # slot out of range
                 ([1], [V], [20]), ([1], [-1], [20]),   # token out of range
                 ([1], [2], [24]), ([1], [2], [-1]),    # position outside the slot
                 ([], [], []), (list(range(3)) * 86, [0] * 258, [0] * 258)]   # n outside [1, KR_MULTI_MAX]
    for sl, tk, ps in bad_steps:
        with pytest.raises(Exception):
            st.step_multi(sl, tk, ps)
    unchanged()
    for fast in [dict(fast=True), dict(fast=False, gemm_fast=True), dict(fast=False, decode_fast=True)]:      # every tolerance bit
        st.set_attention_mode(**fast)
        with pytest.raises(Exception):
            st.step_multi([1], [2], [20])
        with pytest.raises(Exception):
            st.generate_multi([1], [2], [20], 2)
        with pytest.raises(Exception):
            st.step_multi_sample([1], [2], [20])
        st.set_attention_mode(False)
    unchanged()
    with pytest.raises(Exception):
        st.generate_multi([1], [2], [20], 5)                               # 20 + 5 > slot max_seq 24, refused before the first step
    unchanged()
    for n in (-1, 25, 33):
        with pytest.raises(Exception):
            st.save_slot(1, n)
        with pytest.raises(Exception):
            st.load_slot(1, n)
    with pytest.raises(Exception):
        st.save_slot(3, 4)
    st.verify([1, 2], 3)                                                   # a pending verify refuses the steps and the slot copies
    for call in (lambda: st.step_multi([1], [2], [20]), lambda: st.save_slot(1, 4), lambda: st.load_slot(1, 4)):
        with pytest.raises(Exception):
            call()
    st.commit(1)
    unchanged()
    from krasis_amd.ep import ExpertParallel                               # expert parallelism on the engine
    ep = ExpertParallel(eng, eng.num_experts(), 1, 0, return_bf16=False)
    try:
        for call in (lambda: st.step_multi([1], [2], [20]), lambda: st.generate_multi([1], [2], [20], 2), lambda: st.load_slot(1, 20)):
            with pytest.raises(Exception):
                call()
    finally:
        ep.close()
    unchanged()
    st.set_kv_dtype(True)                                                  # slots hold FP16 rows, the store now E4M3
    st.reset_decode_state(d["kv_max"])
    with pytest.raises(Exception):
        st.step_multi([1], [2], [20])
    with pytest.raises(Exception):
        st.load_slot(1, 20)
    st.set_kv_dtype(False)
    unchanged()
    # slots longer than the MLA rope table (its length is the build's kv_max): the table bounds the positions, the slot does not
    st.create_slots(2, 40)
    st.save_slot(1, 20)
    for call in (lambda: st.step_multi([1], [2], [d["kv_max"]]), lambda: st.step_multi([0, 1], [2, 2], [3, d["kv_max"]]),
                 lambda: st.generate_multi([1], [2], [d["kv_max"] - 2], 3)):     # the third token would sit at the table's length
        with pytest.raises(Exception):
            call()
    unchanged()
    ids = st.step_multi([1], [2], [d["kv_max"] - 1])                      # the table's last position runs
    assert len(ids) == 1


def test_native_gguf_experts_are_refused():
    """native-GGUF MoE layers under MLA: their prompt pass is tolerance-only, so neither the steps nor the slot copies run"""
    st, eng, keep, d = _build(kv_max=32, gguf=True, dims=(256, 384, 8, 3, 256, 256))
    st.create_slots(2, 24)
    st.reset_decode_state(d["kv_max"])
    for call in (lambda: st.step_multi([0], [1], [0]), lambda: st.generate_multi([0], [1], [0], 2), lambda: st.save_slot(0, 4),
                 lambda: st.load_slot(0, 4), lambda: st.set_slot_sampler(0, 1, 0.6, 50, 0.95)):
        with pytest.raises(Exception):
            call()


def test_v2lite_widths():
    """DeepSeek-V2-Lite widths: hidden 2048, 16 heads, kv_lora_rank 512, top-6 of 16"""
    st, eng, keep, d = _build(kv_max=160, dims=(2048, 512, 16, 6, 256, 512), nh=16, seed=9)
    rng = np.random.default_rng(2)
    prompts = [_prompt(rng, d, n) for n in (90, 3, 41)]
    firsts = [int(x) for x in rng.integers(0, d["V"], 3)]
    refs = [_reference(st, d, p, f, 2) for p, f in zip(prompts, firsts)]
    st.create_slots(3, 150)
    _fill_slots(st, d, prompts, [[0], [1], [2]])
    toks, pos = _steps_against_refs(st, d, refs, [0, 1, 2], firsts, [len(p) for p in prompts], 2)
    for i, (_, snap) in enumerate(refs):
        st.reset_decode_state(d["kv_max"])
        st.load_slot(i, pos[i])
        _same(_snap(st, d, pos[i]), snap)
