"""The float64 model of one decode layer (tests/decode_f64.py) against the C oracle, on every configuration and token of tests/test_decode_fast_stages_gpu.py.
No GPU: this proves the model, and that the bound the GPU test derives from it cannot hide a wrong kernel.

Per configuration, tap by tap, worst over the tokens:
    e_exact = max |oracle - f64| / max |f64|        the reference's own summation order against the sums carried in float64
    e_tree  = max |tree   - f64| / max |f64|        the same code with f32 pairwise sums: a model of what KR_DECODE_FAST does
(a) the oracle driven through decode_f64.step is the oracle of tests/oracle_decode.py bit for bit (same control flow), the float64 model selects the same experts
    on every counted token, and each of its taps is within CAP / 4 of the oracle's;
(c) 4 * max(e_exact, e_tree) <= CAP = 2e-4 for every value tap: a tenth of the whole-model bound of tests/test_decode_fast_gpu.py.
Router ids count on a token only where the float64 model's k-th and (k+1)-th selection scores differ by more than 100 * e_exact(router logits) of the largest
score; at most 10 % of all tokens may be left out (asserted over the whole case list)."""
import functools

import numpy as np
import pytest

from tests import decode_f64 as M

F = np.float32


@functools.lru_cache(maxsize=None)
def measure(ci):
    case = M.CASES[ci]
    st, eng, orc, keep, d = M.build_case(case, oracle_only=True)
    fp8 = bool(case.get("fp8"))
    e_exact, e_tree, counted, same_ids, hot_p = {}, {}, [], [], None
    for tok, pos in M.tokens(case):
        tr = M.step(orc, tok, pos, M.Ref(), fp8)
        n64 = M.Num(False)
        t64 = M.step(orc, tok, pos, n64, fp8)
        tt = M.step(orc, tok, pos, M.Num(True), fp8)
        for name in case["taps"]:
            if name in t64:
                e_exact[name] = max(e_exact.get(name, 0.0), M.rel_err(tr[name], t64[name]))
                e_tree[name] = max(e_tree.get(name, 0.0), M.rel_err(tt[name], t64[name]))
        if "router_ids" in t64:
            counted.append(M.router_gap_ok(t64, M.rel_err(tr["router_logits"], t64["router_logits"]), orc.topk))
            same_ids.append(np.array_equal(tr["router_ids"], t64["router_ids"]) and np.array_equal(tt["router_ids"], t64["router_ids"]))
        if "hot" in case and pos == 299:
            hot_p = float(n64.probs[:, case["hot"]].max())
    # the same control flow as the oracle driver: one step of OracleDecode from the same state gives the same logits, bit for bit
    tok, pos = M.tokens(case)[0]
    ref_first = M.step(orc, tok, pos, M.Ref(), fp8)["logits"]
    from oracle import oracle as O
    O.set_kv_fp8(fp8)
    try:
        drv = orc.step(tok, pos)
    finally:
        O.set_kv_fp8(False)
    return dict(e_exact=e_exact, e_tree=e_tree, counted=counted, same_ids=same_ids, hot_p=hot_p, driver_equal=np.array_equal(drv.view(np.uint32), ref_first.view(np.uint32)))


@pytest.mark.parametrize("ci", range(len(M.CASES)), ids=[c["name"] for c in M.CASES])
def test_float64_model_against_the_oracle(ci):
    case, m = M.CASES[ci], measure(ci)
    assert m["driver_equal"], "decode_f64.step(Ref) is not OracleDecode.step"
    for name in m["e_exact"]:
        ex, tr = m["e_exact"][name], m["e_tree"][name]
        print("%-16s %-14s e_exact %.3e  e_tree %.3e" % (case["name"], name, ex, tr))
        assert ex <= M.CAP / 4, (name, ex)                          # (a)
        assert 4.0 * max(ex, tr) <= M.CAP, (name, ex, tr)           # (c)
    for ok, same in zip(m["counted"], m["same_ids"]):
        assert same or not ok, "float64 / tree / oracle selections differ on a token that is no near-tie"
    if "hot" in case:
        assert m["hot_p"] > 0.5, m["hot_p"]      # the scaled K row does carry most of one head's probability


def test_router_ids_count_on_at_least_90_percent_of_the_tokens():
    counted = [ok for ci in range(len(M.CASES)) for ok in measure(ci)["counted"]]
    assert len(counted) > 0 and sum(counted) >= 0.9 * len(counted), (sum(counted), len(counted))
