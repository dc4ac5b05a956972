"""The grouped exact kernel for Q5_K experts (kr_ggs_kernel<GG_Q5_K>, docs/design/46-gguf-q5k-grouped.md): gguf_matmul_rows(13, ...) bit for bit against a numpy
f32 model of gg_row_q5k's two-level chain (tests/test_gguf_q5k_gpu.py::chain over the M rows at once) on each activation row, and the passes of "gguf_exact_pass"
stores with a Q5_K projection against decode_step token by token.  u32 bit patterns, no tolerances.

A unit is one super-block (256 k), requested one ahead; a stage is 1024 k.  K 256: one unit, which asks for itself; 768: the clamp on the last of three; 1280: a
stage boundary and a partial stage.  N 20: padding rows in the last tile; 264: five workgroups and lanes past the grid.  M 1 / 5 / 8 / 11: the chain variants of
2, 4 and 8 rows and a partial second group; 1500 / 2051 rows make the grid large enough for workgroups of 128 and 256 rows."""
import functools

import numpy as np
import pytest

from oracle import oracle as O
import tests.test_gguf_exact_grouped_scalar_gpu as S
import tests.test_gguf_gpu as G
from tests.test_gguf_q5k_gpu import blocks_of, make

pytestmark = pytest.mark.gpu
F = np.float32
U = np.uint32
STORES = [((256, 512, 8, 3, 256, 128), (O.Q5_K, O.Q6_K)),                   # the row-chain kernel on both projections, two types behind one sort
          ((256, 512, 8, 3, 256, 128), (O.Q4_K, O.Q5_K)),                   # image kernel on gate | up, Q5_K down over the f32 hidden rows
          ((512, 512, 8, 3, 256, 128), (O.Q5_K, O.Q5_K))]                   # two super-blocks on gate | up


@pytest.fixture(scope="module")
def eng():
    from krasis_amd import KrasisEngine, ModelConfig
    e = KrasisEngine(); e.configure(ModelConfig(256, 128, 8, 2, 1))
    return e


@functools.lru_cache(maxsize=None)
def _case(K, N, M, bf16):
    rng = np.random.default_rng(7 * K + 3 * N + M)
    blocks = blocks_of(rng, O.Q5_K, N, K)
    X = rng.standard_normal((M, K)).astype(F)
    if bf16:
        X = O.bf16_to_f32(O.f32_to_bf16(X.ravel())).reshape(M, K)      # what the gate | up projections see
    w, xb = O.dequantize(O.Q5_K, blocks, N * K).reshape(N, K // 256, 256), X.reshape(M, K // 256, 256)
    tot = np.zeros((M, N), F)
    for b in range(K // 256):
        s = np.zeros((M, N), F)
        for k in range(256):
            s = s + w[None, :, b, k] * xb[:, None, b, k]               # the product and the sum rounded to f32 one after the other
        tot = tot + s
    return blocks, X, tot


def _check(eng, K, N, M, bf16):
    blocks, X, ref = _case(K, N, M, bf16)
    got = eng.gguf_matmul_rows(O.Q5_K, blocks, N, K, X)
    assert got.shape == (M, N) and np.array_equal(got.view(U), ref.view(U)), float(np.abs(got - ref).max())


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("M", [1, 8, 11])
@pytest.mark.parametrize("N", [8, 20, 264])
@pytest.mark.parametrize("K", [256, 768, 1280])
def test_operator_rows_equal_the_chain_model(eng, K, N, M, bf16):
    _check(eng, K, N, M, bf16)


@pytest.mark.parametrize("K,N,M", [(768, 20, 5), (256, 264, 1500), (256, 264, 2051)])
def test_operator_with_four_chains_and_with_workgroups_of_128_and_256_rows(eng, K, N, M):
    _check(eng, K, N, M, False)


def test_a_row_does_not_depend_on_its_group(eng):
    blocks, X, _ = _case(1280, 20, 11, False)
    at = [9, 2, 5]
    alone, among = eng.gguf_matmul_rows(O.Q5_K, blocks, 20, 1280, X[at]), eng.gguf_matmul_rows(O.Q5_K, blocks, 20, 1280, X)
    assert np.array_equal(alone.view(U), among[at].view(U))


@pytest.mark.parametrize("case", [S.test_step_multi_rows_of_1_5_40_equal_decode_step, S.test_extend_multi_runs_of_1_9_3_equal_decode_steps], ids=["step_multi", "extend_multi"])
@pytest.mark.parametrize("dims,types", STORES)
def test_store_passes_equal_decode_step_and_are_counted(monkeypatch, dims, types, case):
    """the store cases of the Q6_K / Q5_0 file on these stores: step_multi at 1 / 5 / 40 rows with the following step, extend_multi with runs of 1 / 9 / 3, against
    decode_step token by token; the counter grows by the passes with the option at 1 and stays with it at 0; the same bits between the two"""
    monkeypatch.setattr(G, "make", make)      # build's expert maker does not know type 13 (tests/test_gguf_q5k_gpu.py::test_decode_step)
    case(dims, types)
