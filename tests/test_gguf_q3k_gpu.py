"""Q3_K experts (ggml type 11) on the native GGUF path (docs/design/47-gguf-q3k.md).  Neither the reference nor the oracle knows the type's values: one numpy de-quantizer written from ggml's
block definition is, in f32 with the two roundings, the model of the exact chain (bit for bit) and, in float64, the reference of the tolerance tile and of the KR_GEMM_FAST layer."""
import json

import numpy as np
import pytest

from oracle import oracle as O
from tests.test_gguf_gpu import rand_blocks
from tests.test_gguf_q5k_gpu import PK_MOE_COMBINE, PK_MOE_W13, PK_MOE_W2, _expf, bits_equal, eng  # noqa: F401  (eng: the module's engine fixture, dims 256 x 128)
from tests.util import rand_bf16

pytestmark = pytest.mark.gpu
F = np.float32
Q3_K = 11


def blocks_of(rng, t, rows, K):
    """random blocks; Q3_K: raw bytes {hmask[32], qs[64], scales[12], f16 d} with d a finite f16 in 5e-4 .. 4.5e-3, as rand_blocks sets it for the types it knows"""
    if t != Q3_K:
        return rand_blocks(rng, t, rows, K)
    raw = rng.integers(0, 256, size=(rows, K // 256, 110), dtype=np.uint8)
    d = (rng.random((rows, K // 256)) * 4e-3 + 5e-4).astype(np.float16).view(np.uint16)
    raw[:, :, 108] = d & 0xFF; raw[:, :, 109] = d >> 8
    return np.ascontiguousarray(raw.reshape(rows, -1))


def make(rng, H, I, gu_t, dn_t):
    return O.GgufExpert(blocks_of(rng, gu_t, I, H), blocks_of(rng, gu_t, I, H), blocks_of(rng, dn_t, H, I), gu_t, dn_t, H, I)


def dequant(blocks, N, K, dt):
    """w[N, K] = (d * sc) * q in dtype dt, each product rounded to dt: element 128n + 32j + p has q = ((qs[32n + p] >> 2j) & 3 | (hmask[p] >> (4n + j) & 1) << 2) - 4, scale index 8n + 2j + (p >> 4)"""
    b = blocks.reshape(N, K // 256, 110)
    hm, qs, s = b[..., 0:32].astype(np.int64), b[..., 32:96].reshape(N, -1, 2, 1, 32).astype(np.int64), b[..., 96:108].astype(np.int64)
    d = b[..., 108:110].copy().view(np.float16)[..., 0].astype(dt)
    n, j, i = np.arange(2)[:, None, None], np.arange(4)[:, None], np.arange(16)
    q = (((qs >> (2 * j)) & 3) | (((hm[..., None, None, :] >> (4 * n + j)) & 1) << 2)) - 4              # [N, blocks, n, j, p]
    sc = (np.concatenate([s[..., 0:8] & 15, s[..., 0:8] >> 4], axis=-1) | (((s[..., 8 + (i & 3)] >> (2 * (i >> 2))) & 3) << 4)) - 32
    return ((d[..., None] * sc.astype(dt))[..., None] * q.reshape(N, -1, 16, 16).astype(dt)).reshape(N, K)


def chain(blocks, N, K, x):
    """the exact row: per super-block s = 0, s = f32(s + f32(w_k x_k)) in element order, then sum = f32(sum + s)"""
    w = dequant(blocks, N, K, F).reshape(N, K // 256, 256); xb = x.astype(F).reshape(-1, 256)
    tot = np.zeros(N, F)
    for b in range(K // 256):
        s = np.zeros(N, F)
        for k in range(256):
            s = s + w[:, b, k] * xb[b, k]
        tot = tot + s
    return tot


def layer_model(experts, ids, w, act_bf16):
    """moe_forward: Q3_K projections on the chain with libm SiLU and nothing quantised; a Q4_K down on the oracle's integer path over the INT16 image of the hidden vector"""
    x, out = O.bf16_to_f32(act_bf16), np.zeros(experts[0].hidden, F)
    for ex, wi in zip((experts[i] for i in ids), w):
        g, u = chain(ex.gate, ex.inter, ex.hidden, x), chain(ex.up, ex.inter, ex.hidden, x)
        h = (g / (F(1.0) + np.array([_expf(float(v)) for v in -g], F))) * u
        dn = chain(ex.down, ex.hidden, ex.inter, h) if ex.down_type == Q3_K else O.gguf_matvec_int(ex.down_type, ex.down, *O.gguf_quant_f32(h), ex.hidden, ex.inter)
        out = out + F(wi) * dn
    return out


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("N", [8, 20])
@pytest.mark.parametrize("K", [256, 768, 2304])
def test_exact_chain_bit_equal(eng, K, N, bf16):
    rng = np.random.default_rng(K + N)
    blocks, x = blocks_of(rng, Q3_K, N, K), rng.standard_normal(K).astype(F)
    x = O.bf16_to_f32(O.f32_to_bf16(x)) if bf16 else x
    bits_equal(eng.gguf_matvec(Q3_K, blocks, N, K, x, 0), chain(blocks, N, K, x))


@pytest.mark.parametrize("N", [8, 40])
@pytest.mark.parametrize("K", [256, 768, 2304])
def test_tolerance_tile_against_float64(eng, K, N):
    """e_tile <= max(4 e_chain, 4 ulp of f32 at max|y64|), the rule and constants of tests/test_gguf_scalar_tiles_gpu.py"""
    rng = np.random.default_rng(3 * K + N)
    blocks, x = blocks_of(rng, Q3_K, N, K), rng.standard_normal(K).astype(F)
    y64 = dequant(blocks, N, K, np.float64) @ x.astype(np.float64)
    mx = float(np.abs(y64).max())
    err = lambda y: float(np.abs(y.astype(np.float64) - y64).max()) / mx
    e_chain = err(eng.gguf_matvec(Q3_K, blocks, N, K, x, 0))
    bound = max(4.0 * e_chain, 4.0 * float(np.spacing(F(mx))) / mx)
    for parts in (1, 2):
        e_tile = err(eng.gguf_matvec(Q3_K, blocks, N, K, x, parts))
        print(f"K {K} N {N} parts {parts}: e_chain {e_chain:.3e} e_tile {e_tile:.3e} bound {bound:.3e}")
        assert e_tile <= bound, (parts, e_tile, e_chain, bound)


@pytest.mark.parametrize("dn_t", [O.Q4_K, Q3_K])
def test_decode_step(monkeypatch, dn_t):
    """tests/test_decode_gpu.py::build with the expert maker replaced (its rand_blocks does not know type 11; the oracle side is not asked).  Exact mode: one MoE layer bit-equal to the model.
    KR_DECODE_FAST: logits within the mode's 2e-3 of the exact step, the same greedy token, one gate|up launch, one down launch and no combine launch per layer."""
    import tests.test_gguf_gpu as G
    from tests.test_decode_gpu import build
    monkeypatch.setattr(G, "make", make)
    st, eng, orc, keep, d = build(dims=(256, 512, 16, 4, 256, 128), gguf=(Q3_K, dn_t), seed=21)
    rng = np.random.default_rng(2)
    act, ids, w = rand_bf16(rng, (256,)), [3, 0, 12, 7], rng.random(4).astype(F)
    bits_equal(np.frombuffer(eng.moe_forward(0, act.tobytes(), ids, [float(v) for v in w]), F), layer_model(orc.layers[0]["experts"], ids, w, act))

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


@pytest.mark.parametrize("dn_t", [O.Q4_K, Q3_K])
def test_gemm_fast_layer_against_float64(dn_t):
    from tests.test_gguf_fast_native_gpu import engine, prefill, w64 as other64      # and the bounds of its test_layer_against_float64, at its smallest dims
    w64 = lambda t, blocks, N, K: dequant(blocks, N, K, np.float64) if t == Q3_K else other64(t, blocks, N, K)
    H = I = 256; E, k, M = 8, 2, 200
    rng = np.random.default_rng(13 + dn_t)
    experts = [make(rng, H, I, Q3_K, dn_t) for _ in range(E)]
    act = rand_bf16(rng, (M, H)); w = rng.random((M, k)).astype(F)
    ids = np.stack([rng.choice(np.arange(1, 6), k, replace=False) for _ in range(M)]).astype(np.int32)
    ids[:70, 0] = 0; ids[3, 1] = 6; ids[5, 1] = -1; ids[77, :] = -1      # a crowded expert, 7 empty, a skipped slot, an all-skipped row
    x, ref = O.bf16_to_f32(act).astype(np.float64), np.zeros((M, H))
    for e, ex in enumerate(experts):
        rows, slots = np.nonzero(ids == e)
        g, u = x[rows] @ w64(Q3_K, ex.gate, I, H).T, x[rows] @ w64(Q3_K, ex.up, I, H).T
        ref[rows] += w[rows, slots, None].astype(np.float64) * ((g / (1.0 + np.exp(-g)) * u) @ w64(dn_t, ex.down, H, I).T)
    def first_fast_call(exs, gu_t):      # the result and what device_bytes() grew by
        eng = engine(exs, None, H, I, k, gu_t, dn_t)
        before = eng.device_bytes()
        return eng, prefill(eng, act, ids, w, True), eng.device_bytes() - before
    eng, got, grew = first_fast_call(experts, Q3_K)
    # the Q3_K projections build no copy.  A Q4_K down keeps the re-tiled copy of its own form: the growth is then exactly that of a layer whose gate | up is Q6_K, known to build none
    assert grew == (0 if dn_t == Q3_K else first_fast_call([make(rng, H, I, O.Q6_K, dn_t) for _ in range(E)], O.Q6_K)[2]), grew
    assert not np.array_equal(got, prefill(eng, act, ids, w, False)), "the tolerance pass returned the exact pass's bits"
    rms = float(np.sqrt(((got - ref) ** 2).mean() / (ref ** 2).mean())); mx = float(np.abs(got - ref).max() / np.abs(ref).max())
    print(f"down {dn_t}: rel RMS {rms:.3e}  max|diff|/max|ref| {mx:.3e}")
    assert np.isfinite(got).all() and 2e-5 < rms <= 1.5e-3 and mx <= 1e-2 and not got[77].any(), (rms, mx)


def test_loader_native(tmp_path):
    from krasis_amd import KrasisEngine
    from tests.test_loader import _GGML, write_gguf
    H, I, E = 256, 256, 3
    rng = np.random.default_rng(4)
    experts = [make(rng, H, I, Q3_K, O.Q4_K) for _ in range(E)]
    cat = lambda name: np.concatenate([getattr(ex, name).reshape(-1) for ex in experts]).tobytes()
    write_gguf(str(tmp_path / "m.gguf"), [(f"blk.1.ffn_{p}_exps.weight", dims, t, cat(p)) for p, dims, t in (("gate", (H, I, E), Q3_K), ("up", (H, I, E), Q3_K), ("down", (I, H, E), _GGML["Q4_K"][0]))])
    (tmp_path / "config.json").write_text(json.dumps({"hidden_size": H, "moe_intermediate_size": I, "n_routed_experts": E, "num_experts_per_tok": 2,
                                                      "num_hidden_layers": 2, "first_k_dense_replace": 1, "n_shared_experts": 0}))
    eng = KrasisEngine()
    eng.load(str(tmp_path), gguf_path=str(tmp_path / "m.gguf"), gguf_native=True)
    act, ids, w = rand_bf16(rng, (H,)), [2, 0], np.array([0.75, 0.5], F)
    bits_equal(np.frombuffer(eng.moe_forward(0, act.tobytes(), ids, [float(v) for v in w]), F), layer_model(experts, ids, w, act))
