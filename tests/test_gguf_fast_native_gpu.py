"""KR_GEMM_FAST on the native lane records of Q6_K and Q5_0 experts (kr_gfh_gemm_kernel, docs/design/42-gguf-fast-native.md): the prompt pass of layers that
hold the two types, per projection, against float64 -- and that it builds no copy of them."""
import numpy as np
import pytest

from oracle import oracle as O
from tests.test_gguf_gpu import make
from tests.test_gguf_scalar_tiles_gpu import dot64
from tests.util import rand_bf16

pytestmark = pytest.mark.gpu
RSF = 1.5


def w64(t, blocks, N, K):
    if t in (O.Q5_0, O.Q6_K):
        return dot64(t, blocks, N, K, np.eye(K))
    return O.dequantize(t, blocks, N * K).astype(np.float64).reshape(N, K)


def expert64(ex, x):
    H, I = ex.hidden, ex.inter
    g, u = x @ w64(ex.gate_up_type, ex.gate, I, H).T, x @ w64(ex.gate_up_type, ex.up, I, H).T
    return (g / (1.0 + np.exp(-g)) * u) @ w64(ex.down_type, ex.down, H, I).T


def engine(experts, sh, H, I, k, gu_t, dn_t):
    from krasis_amd import KrasisEngine, ModelConfig
    eng = KrasisEngine(); eng.configure(ModelConfig(H, I, len(experts), k, 1, 1 if sh else 0, RSF))
    for e, ex in enumerate(experts):
        eng.load_gguf_expert(0, e, ex.gate, ex.up, ex.down, gu_t, dn_t, I)
    if sh:
        eng.load_gguf_expert(0, -1, sh.gate, sh.up, sh.down, gu_t, dn_t, I)
    return eng


def prefill(eng, act, ids, w, fast):
    import torch
    from krasis_amd import _lib
    from krasis_amd._lib import check
    M, k = ids.shape
    xd = torch.from_numpy(act.view(np.int16)).cuda(); idd = torch.from_numpy(ids).cuda(); wd = torch.from_numpy(w).cuda()
    got = torch.empty((M, act.shape[1]), dtype=torch.float32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream or 1
    check(eng._lib.kr_moe_set_gemm_mode(eng._h, 1 if fast else 0))
    check(eng._lib.kr_moe_prefill(eng._h, 0, xd.data_ptr(), idd.data_ptr(), wd.data_ptr(), got.data_ptr(), M, k, _lib.KR_OUT_F32, 0, st))
    check(eng._lib.kr_moe_set_gemm_mode(eng._h, 0))
    torch.cuda.synchronize()
    return got.cpu().numpy()


@pytest.mark.parametrize("H,I,gu_t,dn_t,shared", [
    (256, 256, O.Q4_K, O.Q6_K, False),      # one super-block
    (512, 768, O.Q6_K, O.Q6_K, True),       # three stages, the new form in every position and on dense rows
    (256, 32, O.Q4_K, O.Q5_0, False),       # a single block: a ragged first stage
    (256, 160, O.Q8_0, O.Q5_0, False),      # five blocks: a ragged block group
    (384, 256, O.Q5_0, O.Q6_K, False),      # twelve blocks: one full group and a ragged one, on gate | up (the engine takes hidden sizes of whole 128s only)
    (512, 1408, O.Q4_K, O.Q5_0, False),     # V2-Lite's own intermediate size
])
def test_layer_against_float64(H, I, gu_t, dn_t, shared):
    """kr_moe_prefill under kr_moe_set_gemm_mode(1) against a float64 model of the layer (de-quantised matrices, silu(g) * u, weighted routed sum times the
    routed scaling factor, plus the shared expert).  Expert 7 receives no row, expert 6 one, expert 0 a full row tile and a ragged second one; one id is -1 and
    row 77 is skipped whole.  Bounds: the mode's own (test_moe_prefill_q4k_tolerance_form: f16 activations 2^-11, f16 scales 2^-12) -- relative RMS <= 1.5e-3,
    max|diff| <= 1e-2 max|ref|, the skipped row exactly zero; and relative RMS > 2e-5.  The oracle's exact moe_forward_gguf is held against the same float64
    rows: a layer of the two scalar types alone stays below 2e-5 (measured 4e-7 .. 8e-7), so there the lower bound tells the forms apart; with Q4_K / Q8_0 gate | up
    the exact layer is itself 3e-5 .. 9e-5 away (INT16 activation images, 2^-15) -- held below 1e-3 only as a check of the float64 model -- and the lower bound
    cannot: for every case the tolerance pass must also differ in bits from the exact pass of the same engine, which the pass these layers took before did not.
    Measured on MI355X (relative RMS, max), in the order of the cases: 9.10e-4, 7.91e-4; 5.59e-4, 5.84e-4; 8.62e-4, 8.21e-4;
    4.60e-4, 5.13e-4; 4.93e-4, 6.03e-4; 6.95e-4, 9.00e-4."""
    E, k, M = 8, 2, 200
    rng = np.random.default_rng(H + I + gu_t * 7 + dn_t)
    experts = [make(rng, H, I, gu_t, dn_t) for _ in range(E)]
    sh = make(rng, H, I, gu_t, dn_t) if shared else None
    act = rand_bf16(rng, (M, H)); w = rng.random((M, k)).astype(np.float32)
    ids = np.stack([rng.choice(np.arange(1, 6), k, replace=False) for _ in range(M)]).astype(np.int32)
    ids[:70, 0] = 0; ids[3, 1] = 6; ids[5, 1] = -1; ids[77, :] = -1
    x = O.bf16_to_f32(act).astype(np.float64)
    ref = np.zeros((M, H))
    for e in range(E):
        rows, slots = np.nonzero(ids == e)
        if len(rows):
            ref[rows] += w[rows, slots, None].astype(np.float64) * expert64(experts[e], x[rows])
    if shared:      # the routed scaling factor enters with the shared expert only, as in moe_forward_gguf
        ref = RSF * ref + expert64(sh, x)
    for b in (0, 3, 5):
        sel = [(experts[i], wi) for i, wi in zip(ids[b], w[b]) if i >= 0]
        orc = O.moe_forward_gguf([s[0] for s in sel], [s[1] for s in sel], act[b], sh, RSF)
        e_orc = float(np.sqrt(((orc - ref[b]) ** 2).mean() / (ref[b] ** 2).mean()))
        print(f"row {b}: oracle's exact layer against float64 {e_orc:.3e}")
        assert e_orc < (2e-5 if gu_t in (O.Q5_0, O.Q6_K) else 1e-3)
    eng = engine(experts, sh, H, I, k, gu_t, dn_t)
    got = prefill(eng, act, ids, w, True)
    assert not np.array_equal(got, prefill(eng, act, ids, w, False)), "the tolerance pass returned the exact pass's bits"
    rms = float(np.sqrt(((got - ref) ** 2).mean() / (ref ** 2).mean())); mx = float(np.abs(got - ref).max() / np.abs(ref).max())
    print(f"types {gu_t}|{dn_t} H={H} I={I} shared={shared}: rel RMS {rms:.3e}  max|diff|/max|ref| {mx:.3e}")
    assert np.isfinite(got).all() and rms <= 1.5e-3 and mx <= 1e-2, (rms, mx)
    assert rms > 2e-5, ("the tolerance form did not run", rms)
    if not shared:
        assert not got[77].any()


def test_no_derived_copy():
    """the tolerance pass leaves the reported weight bytes of a Q6_K | Q5_0 layer as they were; a Q4_K | Q6_K and a Q6_K | Q4_K layer grow by the Q4_K copies
    alone: together by exactly what the Q4_K | Q4_K layer of the same shapes grows by"""
    H = I = 256
    grow = {}
    for gu_t, dn_t in ((O.Q6_K, O.Q5_0), (O.Q4_K, O.Q6_K), (O.Q6_K, O.Q4_K), (O.Q4_K, O.Q4_K)):
        rng = np.random.default_rng(5)
        experts = [make(rng, H, I, gu_t, dn_t) for _ in range(2)]
        eng = engine(experts, None, H, I, 2, gu_t, dn_t)
        before = eng.device_bytes()
        prefill(eng, rand_bf16(rng, (4, H)), np.tile(np.array([[0, 1]], np.int32), (4, 1)), np.ones((4, 2), np.float32), True)
        grow[gu_t, dn_t] = eng.device_bytes() - before
    assert grow[O.Q6_K, O.Q5_0] == 0
    assert grow[O.Q4_K, O.Q6_K] > 0 and grow[O.Q6_K, O.Q4_K] > 0
    assert grow[O.Q4_K, O.Q6_K] + grow[O.Q6_K, O.Q4_K] == grow[O.Q4_K, O.Q4_K]


@pytest.mark.parametrize("dims,types", [((256, 512, 16, 4, 256, 128), (O.Q4_K, O.Q6_K)), ((256, 512, 16, 4, 160, 128), (O.Q6_K, O.Q5_0)),
                                        ((512, 512, 8, 2, 256, 128), (O.Q5_0, O.Q6_K))])
def test_whole_model_prompt_pass(dims, types):
    """prefill of 70 tokens under set_attention_mode(False, gemm_fast=True) against the same store's exact prefill: last-row logits within the 1e-2 relative
    tests/test_gemm_fast_gpu.py allows its prompt pass, the same greedy token where the exact top-two margin exceeds that bound.  Measured: 2.68e-3, 2.90e-3, 4.65e-3 (these blocks carry random
    scale bytes, so the expert branch dominates the residual stream; six prompts per pair gave 1.9e-3 .. 8.7e-3, and one of the 18 an expert swap at a router
    near-tie: docs/design/42-gguf-fast-native.md)"""
    from tests.test_decode_gpu import build
    st, eng, orc, keep, d = build(dims=dims, gguf=types, seed=21, kv_max=128)
    toks = [int(t) for t in np.random.default_rng(5).integers(0, d["V"], 70)]
    res = {}
    for fast in (False, True):
        d["reset"]()
        st.set_attention_mode(False, gemm_fast=fast)
        lg = np.empty(d["V"], np.float32)
        st.prefill(toks, 0, lg.ctypes.data)
        res[fast] = lg
    exact, fast = res[False], res[True]
    rel = float(np.abs(fast - exact).max() / np.abs(exact).max())
    print(f"types {types}: last-row logits rel {rel:.3e}")
    assert np.isfinite(fast).all() and rel <= 1e-2, rel
    top = np.sort(exact)[-2:]
    if top[1] - top[0] > 1e-2 * np.abs(exact).max():
        assert int(np.argmax(fast)) == int(np.argmax(exact))
