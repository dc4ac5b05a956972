"""Q5_K experts (ggml type 13) on the native GGUF path (docs/design/45-gguf-q5k.md): the exact row chain bit for bit against a numpy f32 model of the reference's
scalar Q4_K row over dequant_q5_k's values, the tolerance tile and the KR_GEMM_FAST layer against float64, the decode step in both modes, and the loader.
Measured on MI355X: chain 2.4e-7 .. 7.8e-7 and tile 1.1e-7 .. 8.9e-7 of max|y64| (worst tile / bound 0.29); KR_DECODE_FAST logits within 1.4e-5 of the exact step;
KR_GEMM_FAST layer relative RMS 5.5e-4 (Q6_K down), 1.9e-4 (Q5_K down)."""
import ctypes
import json

import numpy as np
import pytest

from oracle import oracle as O
from tests.test_gguf_gpu import rand_blocks
from tests.util import rand_bf16

pytestmark = pytest.mark.gpu
F = np.float32
PK_MOE_W13, PK_MOE_W2, PK_MOE_COMBINE = 9, 10, 11      # positions in the PK_* enum of krasis_amd/csrc/kr_decode_internal.h
_expf = ctypes.CDLL("libm.so.6").expf
_expf.restype, _expf.argtypes = ctypes.c_float, [ctypes.c_float]


def blocks_of(rng, t, rows, K):
    """random blocks; Q5_K: d and dmin as tests/test_gguf_gpu.py::rand_blocks sets them for Q4_K (that function does not know type 13)"""
    if t != O.Q5_K:
        return rand_blocks(rng, t, rows, K)
    raw = rng.integers(0, 256, size=(rows, K // 256, 176), dtype=np.uint8)
    d = (rng.random((rows, K // 256)) * 4e-3 + 5e-4).astype(np.float16).view(np.uint16)
    dm = (rng.random((rows, K // 256)) * 2e-3 + 1e-4).astype(np.float16).view(np.uint16)
    raw[:, :, 0] = d & 0xFF; raw[:, :, 1] = d >> 8; raw[:, :, 2] = dm & 0xFF; raw[:, :, 3] = dm >> 8
    return np.ascontiguousarray(raw.reshape(rows, -1))


def make(rng, H, I, gu_t, dn_t):
    return O.GgufExpert(blocks_of(rng, gu_t, I, H), blocks_of(rng, gu_t, I, H), blocks_of(rng, dn_t, H, I), gu_t, dn_t, H, I)


def chain(t, blocks, N, K, x):
    """the exact row.  Q5_K: per super-block s = 0, s = f32(s + f32(w_k x_k)) in element order, then sum = f32(sum + s), over the values of dequant_q5_k
    (oracle.dequantize == gguf.rs:740); the other types: the oracle's scalar row"""
    if t != O.Q5_K:
        return O.gguf_matvec_f32(t, blocks, x, N, K)
    w = O.dequantize(t, blocks, N * K).reshape(N, K // 256, 256); xb = x.astype(F).reshape(-1, 256)
    tot = np.zeros(N, F)
    for b in range(K // 256):
        s = np.zeros(N, F)
        for k in range(256):
            s = s + w[:, b, k] * xb[b, k]
        tot = tot + s
    return tot


def w64(t, blocks, N, K):
    """the block values formed in float64 from d, dmin, the 6-bit scales and minima and the 5-bit codes"""
    if t != O.Q5_K:
        from tests.test_gguf_fast_native_gpu import w64 as other
        return other(t, blocks, N, K)
    b = blocks.reshape(N, K // 256, 176)
    d, dmin = (b[..., i:i + 2].copy().view(np.float16)[..., 0].astype(np.float64) for i in (0, 2))
    s = b[..., 4:16].astype(np.int64); qh = b[..., None, 16:48].astype(np.int64); qs = b[..., 48:176].reshape(N, -1, 4, 32).astype(np.int64)
    sc = np.concatenate([s[..., 0:4] & 63, (s[..., 8:12] & 0xF) | ((s[..., 0:4] >> 6) << 4)], axis=-1)      # get_scale_min_k4
    mn = np.concatenate([s[..., 4:8] & 63, (s[..., 8:12] >> 4) | ((s[..., 4:8] >> 6) << 4)], axis=-1)
    j = np.arange(4)[:, None]
    q = np.stack([(qs & 0xF) | (((qh >> (2 * j)) & 1) << 4), (qs >> 4) | (((qh >> (2 * j + 1)) & 1) << 4)], axis=3).reshape(N, -1, 8, 32)
    return ((d[..., None] * sc)[..., None] * q - (dmin[..., None] * mn)[..., None]).reshape(N, K)


def layer_chain(experts, ids, w, act_bf16):
    """moe_forward on the scalar path: nothing is quantised, libm SiLU (expert_forward_gguf), the weighted sum in routing order"""
    x, out = O.bf16_to_f32(act_bf16), np.zeros(experts[0].hidden, F)
    for ex, wi in zip((experts[i] for i in ids), w):
        g, u = chain(ex.gate_up_type, ex.gate, ex.inter, ex.hidden, x), chain(ex.gate_up_type, ex.up, ex.inter, ex.hidden, x)
        e = np.array([_expf(float(v)) for v in -g], F)
        out = out + F(wi) * chain(ex.down_type, ex.down, ex.hidden, ex.inter, (g / (F(1.0) + e)) * u)
    return out


def bits_equal(got, ref):
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), float(np.abs(got - ref).max())


@pytest.fixture(scope="module")
def eng():
    from krasis_amd import KrasisEngine, ModelConfig
    e = KrasisEngine(); e.configure(ModelConfig(256, 128, 8, 2, 1))
    return e


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("N", [8, 20])
@pytest.mark.parametrize("K", [256, 768, 2304])
def test_exact_chain_bit_equal(eng, K, N, bf16):
    rng = np.random.default_rng(K + N)
    blocks, x = blocks_of(rng, O.Q5_K, N, K), rng.standard_normal(K).astype(F)
    if bf16:
        x = O.bf16_to_f32(O.f32_to_bf16(x))
    bits_equal(eng.gguf_matvec(O.Q5_K, blocks, N, K, x, 0), chain(O.Q5_K, blocks, N, K, x))


@pytest.mark.parametrize("N", [8, 40])
@pytest.mark.parametrize("K", [256, 768, 2304])
def test_tolerance_tile_against_float64(eng, K, N):
    """e_tile <= max(4 e_chain, 4 ulp of f32 at max|y64|), the rule and constants of tests/test_gguf_scalar_tiles_gpu.py"""
    rng = np.random.default_rng(3 * K + N)
    blocks, x = blocks_of(rng, O.Q5_K, N, K), rng.standard_normal(K).astype(F)
    y64 = w64(O.Q5_K, blocks, N, K) @ x.astype(np.float64)
    mx = float(np.abs(y64).max())
    err = lambda y: float(np.abs(y.astype(np.float64) - y64).max()) / mx
    e_chain = err(eng.gguf_matvec(O.Q5_K, blocks, N, K, x, 0))
    bound = max(4.0 * e_chain, 4.0 * float(np.spacing(F(mx))) / mx)
    for parts in (1, 2):
        e_tile = err(eng.gguf_matvec(O.Q5_K, blocks, N, K, x, parts))
        print(f"K {K} N {N} parts {parts}: e_chain {e_chain:.3e} e_tile {e_tile:.3e} bound {bound:.3e}")
        assert e_tile <= bound, (parts, e_tile, e_chain, bound)


@pytest.mark.parametrize("dn_t", [O.Q6_K, O.Q5_K])
def test_decode_step(monkeypatch, dn_t):
    """tests/test_decode_gpu.py::build draws its experts from tests.test_gguf_gpu.make, whose rand_blocks does not know type 13, and its oracle has no row for the
    type: the expert maker is replaced for the call and the oracle side is not asked.  Exact mode: one MoE layer bit-equal to the chain model.  KR_DECODE_FAST: logits
    within the mode's 2e-3 of the exact step, the same greedy token, one gate|up launch, one down launch and no combine launch per layer."""
    import tests.test_gguf_gpu as G
    from tests.test_decode_gpu import build
    monkeypatch.setattr(G, "make", make)
    st, eng, orc, keep, d = build(dims=(256, 512, 16, 4, 256, 128), gguf=(O.Q5_K, dn_t), seed=21)
    rng = np.random.default_rng(2)
    act, ids, w = rand_bf16(rng, (256,)), [3, 0, 12, 7], rng.random(4).astype(F)
    bits_equal(np.frombuffer(eng.moe_forward(0, act.tobytes(), ids, [float(v) for v in w]), F), layer_chain(orc.layers[0]["experts"], ids, w, act))

    def run(toks):      # three steps; toks None: each step's greedy token feeds the next
        d["reset"]()
        out = []
        for i, pos in enumerate((5, 6, 7)):
            out.append(np.empty(d["V"], F))
            st.decode_step(toks[i] if toks else (int(np.argmax(out[-2])) if i else 7), pos, out[-1].ctypes.data)
        return out
    st.set_use_graph(True)
    exact = run(None)
    st.set_attention_mode(False, decode_fast=True)
    for pos, (a, b) in enumerate(zip(run([7] + [int(np.argmax(lg)) for lg in exact[:2]]), exact)):
        err = float(np.abs(a - b).max() / np.abs(b).max())
        print(f"down {dn_t} step {pos}: logits rel {err:.3e}")
        assert err <= 2e-3 and int(np.argmax(a)) == int(np.argmax(b)), (pos, err)
    cnt = [c for _, c in st.profile_step(int(np.argmax(exact[2])), 8)]
    assert (cnt[PK_MOE_W13], cnt[PK_MOE_W2], cnt[PK_MOE_COMBINE]) == (len(d["kinds"]), len(d["kinds"]), 0)


@pytest.mark.parametrize("dn_t", [O.Q6_K, O.Q5_K])
def test_gemm_fast_layer_against_float64(dn_t):
    """the shape and bounds of tests/test_gguf_fast_native_gpu.py::test_layer_against_float64 at its smallest dims"""
    from tests.test_gguf_fast_native_gpu import engine, prefill
    H = I = 256; E, k, M = 8, 2, 200
    rng = np.random.default_rng(13 + dn_t)
    experts = [make(rng, H, I, O.Q5_K, dn_t) for _ in range(E)]
    act = rand_bf16(rng, (M, H)); w = rng.random((M, k)).astype(F)
    ids = np.stack([rng.choice(np.arange(1, 6), k, replace=False) for _ in range(M)]).astype(np.int32)
    ids[:70, 0] = 0; ids[3, 1] = 6; ids[5, 1] = -1; ids[77, :] = -1
    x = O.bf16_to_f32(act).astype(np.float64)
    ref = np.zeros((M, H))
    for e, ex in enumerate(experts):
        rows, slots = np.nonzero(ids == e)
        g, u = x[rows] @ w64(O.Q5_K, ex.gate, I, H).T, x[rows] @ w64(O.Q5_K, ex.up, I, H).T
        ref[rows] += w[rows, slots, None].astype(np.float64) * ((g / (1.0 + np.exp(-g)) * u) @ w64(dn_t, ex.down, H, I).T)
    eng = engine(experts, None, H, I, k, O.Q5_K, dn_t)
    before = eng.device_bytes()
    got = prefill(eng, act, ids, w, True)
    assert eng.device_bytes() == before
    assert not np.array_equal(got, prefill(eng, act, ids, w, False)), "the tolerance pass returned the exact pass's bits"
    rms = float(np.sqrt(((got - ref) ** 2).mean() / (ref ** 2).mean())); mx = float(np.abs(got - ref).max() / np.abs(ref).max())
    print(f"down {dn_t}: rel RMS {rms:.3e}  max|diff|/max|ref| {mx:.3e}")
    assert np.isfinite(got).all() and 2e-5 < rms <= 1.5e-3 and mx <= 1e-2 and not got[77].any(), (rms, mx)


def test_loader_native(tmp_path):
    from krasis_amd import KrasisEngine
    from tests.test_loader import _GGML, write_gguf
    H, I, E = 256, 256, 3
    rng = np.random.default_rng(4)
    experts = [make(rng, H, I, O.Q5_K, O.Q6_K) for _ in range(E)]
    cat = lambda name: np.concatenate([getattr(ex, name).reshape(-1) for ex in experts]).tobytes()
    write_gguf(str(tmp_path / "m.gguf"), [(f"blk.1.ffn_{p}_exps.weight", dims, _GGML[t][0], cat(p)) for p, dims, t in (("gate", (H, I, E), "Q5_K"), ("up", (H, I, E), "Q5_K"), ("down", (I, H, E), "Q6_K"))])
    (tmp_path / "config.json").write_text(json.dumps({"hidden_size": H, "moe_intermediate_size": I, "n_routed_experts": E, "num_experts_per_tok": 2,
                                                      "num_hidden_layers": 2, "first_k_dense_replace": 1, "n_shared_experts": 0}))
    eng = KrasisEngine()
    eng.load(str(tmp_path), gguf_path=str(tmp_path / "m.gguf"), gguf_native=True)
    act, ids, w = rand_bf16(rng, (H,)), [2, 0], np.array([0.75, 0.5], F)
    bits_equal(np.frombuffer(eng.moe_forward(0, act.tobytes(), ids, [float(v) for v in w]), F), layer_chain(experts, ids, w, act))
