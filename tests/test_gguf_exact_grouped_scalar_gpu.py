"""The grouped exact kernel for Q6_K / Q5_0 experts (krasis_amd/csrc/kr_gguf_group.hip, docs/design/43-gguf-exact-grouped-scalar.md): the stand-alone
operator gguf_matmul_rows bit for bit against the oracle's scalar row on each activation row alone, and the passes of "gguf_exact_pass" stores that hold such
matrices against decode_step token by token.  u32 bit patterns, no tolerances.

The kernel stages 1024 k of the group's rows at a time and requests 256 k (a Q6_K super-block, a Q5_0 group of 8 blocks) ahead: K 1280 / 1408 cross one
stage boundary with a partial remainder, K 768 / 288 make the request-ahead clamp / leave a ragged last group.  A workgroup takes 64, 128 or 256 output
rows by the size of the grid: the small shapes all take 64 (N 264 is five workgroups), so two cases with many rows reach 128 and 256."""
import numpy as np
import pytest

from oracle import oracle as O
from tests.slots import Gqa, toks as _toks
from tests.test_decode_gpu import build
from tests.test_gguf_gpu import rand_blocks
from tests.test_gguf_exact_pass_gpu import _assert_group, _rows, _step_group
from tests.test_multi_extend_gpu import _assert_rows, _run_reference

pytestmark = pytest.mark.gpu
F = np.float32
U = np.uint32
OPERATOR = [(O.Q6_K, 256), (O.Q6_K, 768), (O.Q6_K, 1280), (O.Q5_0, 32), (O.Q5_0, 288), (O.Q5_0, 1408)]
MIXED = ((256, 512, 8, 3, 256, 128), (O.Q4_K, O.Q6_K))                      # both grouped kernels behind one sort
STORES = [MIXED,
          ((256, 512, 8, 3, 160, 128), (O.Q6_K, O.Q5_0)),                   # I = 160: five blocks, a ragged group
          ((512, 512, 8, 3, 256, 128), (O.Q5_0, O.Q6_K))]                   # two Q5_0 block groups on gate | up
NAME = "gguf_grouped_scalar"


@pytest.fixture(scope="module")
def eng():
    from krasis_amd import KrasisEngine, ModelConfig
    e = KrasisEngine(); e.configure(ModelConfig(256, 128, 8, 2, 1))
    return e


def _case(t, K, N, M, bf16):
    rng = np.random.default_rng(7 * K + 3 * N + M + t)
    blocks = rand_blocks(rng, t, N, K)
    X = rng.standard_normal((M, K)).astype(F)
    if bf16:
        X = O.bf16_to_f32(O.f32_to_bf16(X.ravel())).reshape(M, K)      # what the gate | up projections see
    return blocks, X, np.stack([O.gguf_matvec_f32(t, blocks, x, N, K) for x in X])


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("M", [1, 8, 11])
@pytest.mark.parametrize("N", [8, 20, 264])
@pytest.mark.parametrize("t,K", OPERATOR)
def test_operator_rows_equal_the_oracle_row(eng, t, K, N, M, bf16):
    blocks, X, ref = _case(t, K, N, M, bf16)
    got = eng.gguf_matmul_rows(t, blocks, N, K, X)
    assert got.shape == (M, N) and np.array_equal(got.view(U), ref.view(U)), float(np.abs(got - ref).max())


@pytest.mark.parametrize("t,K,M", [(O.Q6_K, 256, 1500), (O.Q5_0, 288, 1500), (O.Q6_K, 256, 2051), (O.Q5_0, 288, 2051)])
def test_operator_with_workgroups_of_128_and_256_rows(eng, t, K, M):
    blocks, X, ref = _case(t, K, 264, M, False)
    assert np.array_equal(eng.gguf_matmul_rows(t, blocks, 264, K, X).view(U), ref.view(U))


@pytest.mark.parametrize("t,K", [(O.Q6_K, 1280), (O.Q5_0, 1408)])
def test_a_row_does_not_depend_on_its_group(eng, t, K):
    blocks, X, _ = _case(t, K, 20, 11, False)
    at = [9, 2, 5]
    alone, among = eng.gguf_matmul_rows(t, blocks, 20, K, X[at]), eng.gguf_matmul_rows(t, blocks, 20, K, X)
    assert np.array_equal(alone.view(U), among[at].view(U))


def test_operator_refusals(eng):
    blocks = rand_blocks(np.random.default_rng(0), O.Q6_K, 8, 256)
    for t, K, M in ((O.Q4_K, 256, 2), (O.Q6_K, 128, 2), (O.Q5_0, 48, 2), (O.Q6_K, 256, 0)):
        with pytest.raises(ValueError, match="kr_gguf_matmul_rows"):
            eng.gguf_matmul_rows(t, blocks, 8, K, np.zeros((M, K), F))


def _store(dims, types):
    st, eng, orc, keep, d = build(kv_max=64, dims=dims, gguf=types, seed=11)
    st.set_option("gguf_exact_pass", 1); st.set_option("gguf_exact_grouped_scalar", 1)
    d["_keep"] = (eng, keep)
    return st, d


def _on_then_off(st, passes, run):
    """run(leg) with "gguf_exact_grouped_scalar" 1, then 0: the counter grows by `passes`, then stays; the same bits"""
    got = []
    for on in (1, 0):
        st.set_option("gguf_exact_grouped_scalar", on)
        before = st.multi_path_counts()[NAME]
        got.append(run(1 - on))
        assert st.multi_path_counts()[NAME] - before == (passes if on else 0), on
    return got


@pytest.mark.parametrize("dims,types", STORES)
def test_step_multi_rows_of_1_5_40_equal_decode_step(dims, types):
    st, d = _store(dims, types)
    st.create_slots(92, 16)
    perm = [int(x) for x in np.random.default_rng(3).permutation(40)]
    groups = [([7], 0), ([30, 2, 11, 25, 4], 1), (perm, 6)]                 # several groups per expert, a partial last group, experts with no rows
    prompts, firsts, refs = _rows(st, d, Gqa, 40, groups + [(s, b + 46) for s, b in groups])

    def run(leg):
        out = []
        for seqs, base in groups:
            slots, (ids, lg) = _step_group(st, seqs, base + 46 * leg, prompts, firsts)
            _assert_group(st, seqs, slots, refs, ids, lg)                  # and the following step
            out.append((ids, lg.view(U).copy()))
        return out

    on, off = _on_then_off(st, 6, run)
    assert all(a[0] == b[0] and np.array_equal(a[1], b[1]) for a, b in zip(on, off))


@pytest.mark.parametrize("dims,types", STORES)
def test_extend_multi_runs_of_1_9_3_equal_decode_steps(dims, types):
    st, d = _store(dims, types)
    st.create_slots(8, 40)
    rng = np.random.default_rng(5)
    prompts = [_toks(rng, d, p) for p in (0, 3, 2)]
    runs = [_toks(rng, d, r) for r in (1, 9, 3)]
    slots = ([3, 0, 6], [4, 1, 7])
    refs = [_run_reference(st, d, p, r, [a, b]) for p, r, a, b in zip(prompts, runs, *slots)]

    def run(leg):
        ids, lg = st.extend_multi(slots[leg], runs, [len(p) for p in prompts], logits=True)
        _assert_rows(st, d, refs, slots[leg], ids, lg)
        return ids, lg.view(U).copy()

    on, off = _on_then_off(st, 1, run)
    assert on[0] == off[0] and np.array_equal(on[1], off[1])


def test_single_sequence_prefill_of_33_tokens_in_three_chunks():
    st, d = _store(*MIXED)
    toks = _toks(np.random.default_rng(29), d, 34)
    st.reset_decode_state(d["kv_max"])
    for i, t in enumerate(toks):
        st.decode_step(t, i)
    want = (st.read_logits().view(U).copy(), st.last_token(), Gqa.snap(st, d, 34))
    st.reset_decode_state(d["kv_max"])
    st.set_prefill_chunk(12)
    st.prefill(toks[:33], 0)
    st.decode_step(toks[33], 33)                                            # the step after the pass reads what the pass left
    assert np.array_equal(st.read_logits().view(U), want[0]) and st.last_token() == want[1]
    Gqa.same(Gqa.snap(st, d, 34), want[2])
