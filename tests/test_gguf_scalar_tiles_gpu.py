"""Q5_0 / Q6_K experts on the lane-record layout (krasis_amd/csrc/kr_gguf.hip, kr_gguf_dev.h, docs/design/41-gguf-scalar-tiles.md): the exact row chain bit for
bit against the oracle's scalar row, the tolerance tiles against float64 through kr_gguf_matvec, and the decode step with such matrices in exact mode and under
KR_DECODE_FAST, where a layer with one of them now stays inside the mode's three MoE launches ("gguf_scalar_tiles").

Measured on MI355X, e = max|y - y64| / max|y64| over the operator cases below: the chain 6.1e-8 .. 1.7e-6, the tile 3.4e-8 .. 3.6e-7 (parts 1) / 2.4e-7 (parts 2);
worst ratio of a tile's error to its bound 0.18.  Decode step under KR_DECODE_FAST: logits within 2.9e-4 of the oracle (bound 2e-3)."""
import numpy as np
import pytest

from oracle import oracle as O
from tests.test_decode_gpu import build
from tests.test_gguf_gpu import rand_blocks

pytestmark = pytest.mark.gpu
F = np.float32
SHAPES = [(O.Q6_K, 256), (O.Q6_K, 768), (O.Q6_K, 2304), (O.Q5_0, 32), (O.Q5_0, 160), (O.Q5_0, 288), (O.Q5_0, 1408)]
PK_MOE_W13, PK_MOE_W2, PK_MOE_COMBINE = 9, 10, 11      # positions in the PK_* enum of krasis_amd/csrc/kr_decode_internal.h


def dot64(t, blocks, N, K, x):
    """float64 dot of the exact block values -- d, scales and codes multiplied in float64 -- with x (block layouts: gguf_kernels.rs:572-635)"""
    if t == O.Q5_0:
        b = blocks.reshape(N, K // 32, 22)
        d = b[:, :, 0:2].copy().view(np.float16)[..., 0].astype(np.float64)
        qh = b[:, :, 2:6].copy().view(np.uint32)[..., 0]
        nib = np.concatenate([b[:, :, 6:22] & 0xF, b[:, :, 6:22] >> 4], axis=2).astype(np.int64)
        q = nib | (((qh[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1).astype(np.int64) << 4)
        w = d[:, :, None] * (q - 16)
    else:
        b = blocks.reshape(N, K // 256, 210)
        ql = b[:, :, :128].reshape(N, -1, 2, 2, 32).astype(np.int64)                               # [half][bytes l | 32 + l][l]
        qh = b[:, :, 128:192].reshape(N, -1, 2, 1, 32).astype(np.int64)
        sc = b[:, :, 192:208].copy().view(np.int8).reshape(N, -1, 2, 4, 2).astype(np.float64)      # [half][run g of 32][is]: scale byte is + 2 g
        d = b[:, :, 208:210].copy().view(np.float16)[..., 0].astype(np.float64)
        q = np.stack([ql[:, :, :, 0] & 0xF, ql[:, :, :, 1] & 0xF, ql[:, :, :, 0] >> 4, ql[:, :, :, 1] >> 4], axis=3)      # [half][g][l]: element 32 g + l
        q = q | (((qh >> (2 * np.arange(4))[None, None, None, :, None]) & 3) << 4)
        w = d[:, :, None, None, None] * np.repeat(sc, 16, axis=4) * (q - 32)
    return w.reshape(N, K) @ x.astype(np.float64)


@pytest.fixture(scope="module")
def eng():
    from krasis_amd import KrasisEngine, ModelConfig
    e = KrasisEngine(); e.configure(ModelConfig(256, 128, 8, 2, 1))
    return e


@pytest.mark.parametrize("N", [8, 20])
@pytest.mark.parametrize("t,K", SHAPES)
def test_exact_chain_bit_equal_to_the_oracle_row(eng, t, K, N):
    rng = np.random.default_rng(K + N + t)
    blocks = rand_blocks(rng, t, N, K)
    ex = O.GgufExpert(blocks[:0], blocks[:0], blocks, t, t, N, K)      # the blocks as a down matrix [hidden N, inter K]
    x = rng.standard_normal(K).astype(F)
    ref = O.gguf_matvec_f32(ex.down_type, ex.down, x, N, K)           # the scalar down path of expert_forward_gguf
    got = eng.gguf_matvec(t, blocks, N, K, x, 0)
    assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), float(np.abs(got - ref).max())


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("N", [8, 40])
@pytest.mark.parametrize("t,K", SHAPES)
def test_tolerance_tile_against_float64(eng, t, K, N, bf16):
    """e_tile <= max(4 e_chain, 4 ulp of f32 at max|y64|): two bits of room over the reference's own summation error (the rule and the constants of
    tests/test_decode_fast_stages_gpu.py)"""
    rng = np.random.default_rng(3 * K + N + t)
    blocks = rand_blocks(rng, t, N, K)
    x = rng.standard_normal(K).astype(F)
    if bf16:
        x = O.bf16_to_f32(O.f32_to_bf16(x))      # what the gate | up projections see
    y64 = dot64(t, blocks, N, K, x)
    mx = float(np.abs(y64).max())
    err = lambda y: float(np.abs(y.astype(np.float64) - y64).max()) / mx
    e_chain = err(eng.gguf_matvec(t, blocks, N, K, x, 0))
    bound = max(4.0 * e_chain, 4.0 * float(np.spacing(F(mx))) / mx)
    for parts in (1, 2):
        e_tile = err(eng.gguf_matvec(t, blocks, N, K, x, parts))
        print(f"type {t} K {K} N {N} bf16 {bf16} parts {parts}: e_chain {e_chain:.3e} e_tile {e_tile:.3e} bound {bound:.3e}")
        assert e_tile <= bound, (parts, e_tile, e_chain, bound)


def test_matvec_refuses_what_it_does_not_cover(eng):
    rng = np.random.default_rng(0)
    x = np.zeros(256, F)
    for t, K, parts in ((O.Q4_K, 256, 0), (O.Q6_K, 256, 3), (O.Q6_K, 128, 0), (O.Q5_0, 48, 1)):
        with pytest.raises(ValueError):
            eng.gguf_matvec(t, rand_blocks(rng, O.Q6_K, 8, 256), 8, K, x[:K], parts)


@pytest.mark.parametrize("dims,types", [((256, 512, 16, 4, 256, 128), (O.Q4_K, O.Q6_K)), ((256, 512, 16, 4, 160, 128), (O.Q6_K, O.Q5_0)),
                                        ((512, 512, 8, 2, 256, 128), (O.Q5_0, O.Q6_K))])
def test_decode_step_with_scalar_type_experts(dims, types):
    """exact mode, graph on: logits and greedy token bit-equal to the oracle.  decode_fast: logits within the mode's 2e-3 of the oracle, same greedy token, and per
    MoE layer one gate|up launch, one down launch, no combine launch; with "gguf_scalar_tiles" 0 the launches of before (routed and shared gate|up, one shared
    down, one combine per layer) and again 2e-3"""
    st, eng, orc, keep, d = build(dims=dims, gguf=types, seed=21)
    nL = len(d["kinds"])
    refs, tok = [], 7
    for pos in (5, 6, 7):
        refs.append((tok, pos, orc.step(tok, pos)))
        tok = O.sample_greedy(refs[-1][2])

    def run(exact):
        d["reset"]()
        for tok, pos, ref in refs:
            logits = np.empty(d["V"], F)
            st.decode_step(tok, pos, logits.ctypes.data)
            if exact:
                assert np.array_equal(logits.view(np.uint32), ref.view(np.uint32)), (pos, float(np.abs(logits - ref).max()))
                assert st.last_token() == O.sample_greedy(ref)
            else:
                err = float(np.abs(logits - ref).max() / np.abs(ref).max())
                print(f"types {types} pos {pos}: logits rel {err:.3e}")
                assert err <= 2e-3, (pos, err)
                assert int(np.argmax(logits)) == O.sample_greedy(ref)
        cnt = [c for _, c in st.profile_step(tok, 8)]
        return cnt[PK_MOE_W13], cnt[PK_MOE_W2], cnt[PK_MOE_COMBINE]

    st.set_use_graph(True)
    run(True)
    st.set_attention_mode(False, decode_fast=True)
    assert run(False) == (nL, nL, 0)
    st.set_option("gguf_scalar_tiles", 0)
    assert run(False) == (2 * nL, nL, nL)
