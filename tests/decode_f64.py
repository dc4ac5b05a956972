"""One decode step of a ONE-LAYER model in three arithmetics, with every value the decode store lets a test read back after the step ("taps").

The control flow is tests/oracle_decode.py's OracleDecode.step (src/decode.rs:2690-3520) and the products are the reference's: INT16 activation digits from the
oracle's own quantisers (O.quant_act_int16_f32 / _bf16, O.silu_quant_int16), exact integer group sums, (float)isum * (bf16(w_scale) * a_scale), the poly-5 sigmoid
(O.fast_silu_mul), libm exp / log, the f16 / E4M3 rounding of cache rows.  What differs between the three is how an f32 SUM is formed:

    Ref()        the C oracle's operators: the reference's sequential chains and 8-lane fma accumulators (bit-equal to the exact GPU step)
    Num(False)   every sum carried in float64 and rounded ONCE where the reference stores an f32 -- the value all errors are measured against
    Num(True)    a model of KR_DECODE_FAST: the same code, products rounded to f32 and added in f32 in pairwise (tree) order

Everything that is not a sum (scalar f32 arithmetic on a stored sum, element-wise scaling, RoPE, quantisation decisions, top-k) is the same f32 code in both Num
settings, so the distance between them and to Ref is summation error and what it moves downstream (single INT16 digits, cache-row roundings), nothing else.
libm expf / logf are taken as the float64 function rounded to f32 (glibc's are correctly rounded but for rare last-bit cases).

MLA layers (O.mla_step) are not modelled.

Taps (dict of name -> f32 array), the names of docs/design/07-decode-fast.md:
    conv_new      LA: newest column of the conv state [conv_dim]          recur      LA: recurrent state after the step [nv, dk * dv]
    k_row, v_row  GQA: the appended cache rows, decoded to f32 (k_code / v_code: the stored u16 / u8 words)
    resid_attn    residual after the attention branch: embedding row + out projection
    router_logits, router_w, router_ids   (MoE)                          moe_out    MLP block output (MoE or dense)
    resid_final   resid_attn + moe_out                                     normed     final RMSNorm output          logits
"""
import numpy as np

from oracle import oracle as O

F, D = np.float32, np.float64
_ONE = {}


def _ones(n):
    if n not in _ONE:
        _ONE[n] = np.ones(n, F)
    return _ONE[n]


def expf(x):
    return np.exp(np.asarray(x, D)).astype(F)


def logf(x):
    return np.log(np.asarray(x, D)).astype(F)


def sigmoid_libm(x):      # 1.0f / (1.0f + expf(-x))
    return (F(1.0) / (F(1.0) + expf(-np.asarray(x, F)))).astype(F)


def silu_poly5(x):        # x * sigmoid_poly5(x), avx2.rs:2277
    x = np.ascontiguousarray(x, F)
    return O.fast_silu_mul(x.reshape(-1), _ones(x.size)).reshape(x.shape)


def tree_sum(x, axis=-1):
    """f32 pairwise sum: halves added to halves (zero-padded to a power of two)"""
    x = np.moveaxis(np.asarray(x, F), axis, -1)
    n, p = x.shape[-1], 1
    while p < n:
        p *= 2
    if p != n:
        x = np.concatenate([x, np.zeros(x.shape[:-1] + (p - n,), F)], -1)
    while x.shape[-1] > 1:
        h = x.shape[-1] // 2
        x = x[..., :h] + x[..., h:]
    return x[..., 0]


_E4M3 = None


def e4m3_lut():
    global _E4M3
    if _E4M3 is None:
        _E4M3 = O.e4m3_to_f32(np.arange(256, dtype=np.uint8))
    return _E4M3


def cache_to_f32(codes, fp8):
    codes = np.asarray(codes)
    return e4m3_lut()[codes.astype(np.uint8)] if fp8 else codes.astype(np.uint16).view(np.float16).astype(F)


_UNPACK = {}


def unpack(w, bits):
    """transposed INT4 words [K / 8, N] u32 (nibble j of word kr = k index kr * 8 + j, value - 8) or INT8 [K, N] -> int8 [K, N]; cached per array"""
    key = id(w)
    if key not in _UNPACK:
        if bits == 4:
            w = np.asarray(w, np.uint32)
            q = ((w[:, None, :] >> (np.arange(8, dtype=np.uint32) * np.uint32(4))[None, :, None]) & np.uint32(15)).astype(np.int8) - np.int8(8)
            q = q.reshape(w.shape[0] * 8, w.shape[1])
        else:
            q = np.asarray(w, np.int8)
        _UNPACK[key] = (w, q)      # the source array is kept alive so that its id stays its own
    return _UNPACK[key][1]


class Ref:
    """the C oracle's operators"""
    name = "oracle"

    def add_rmsnorm(self, hid, res, w, eps, first, nbo):
        return O.fused_add_rmsnorm(hid, res, w, eps, first, nbo)

    def matvec_q(self, w, sc, bits, q, s):
        return O.matvec_int4_t(w, sc, q, s) if bits == 4 else O.matvec_int8_t(w, sc, q, s)

    def la(self, L, qkvz, ba, eps):
        c = O.la_conv(qkvz, ba, L["conv_state"], L["conv_w"], L["a_log"], L["dt_bias"], L["scale"], L["nk"], L["nv"], L["dk"], L["dv"], 4)
        ro, rs = O.la_recurrent(L["recur_state"], c["q"], c["k"], c["v"], c["g"], c["beta"], L["nv"], L["dk"], L["dv"])
        return O.gated_rmsnorm_silu(ro, c["z"], L["norm_w"], L["nv"], L["dv"], eps), c["conv_state"], rs

    def gqa(self, L, q, k, v, rope, pos, eps, fp8):
        O.set_kv_fp8(fp8)
        try:
            return O.gqa_step(q, k, v, L["q_norm"], L["k_norm"], L["gated"], L["nh"], L["nkv"], L["hd"], eps, rope[0], rope[1], L["kv_k"], L["kv_v"], pos, L["sm_scale"])
        finally:
            O.set_kv_fp8(False)

    def route(self, gate, hid, k, scoring, esc):
        ids, w, lg = O.route_decode(gate, hid, k, scoring, True, None, esc)
        return lg, ids, w, None

    def routed(self, experts, w, act_bf16):
        return O.moe_forward_unified(experts, np.asarray(w, F), act_bf16)

    def sig(self, x):
        return F(O.sigmoid(float(x), O.SIG_LIBM))


class Num:
    """tree=False: sums in float64, rounded once; tree=True: f32 products in a pairwise f32 tree"""

    def __init__(self, tree):
        self.tree = tree
        self.name = "tree" if tree else "f64"

    def sum(self, a, b=None, axis=-1):
        """sum of a (or of the products a * b) along axis -> f32"""
        if self.tree:
            return tree_sum(np.asarray(a, F) if b is None else np.asarray(a, F) * np.asarray(b, F), axis)
        t = np.asarray(a, D) if b is None else np.asarray(a, D) * np.asarray(b, D)      # an f32 x f32 product is exact in float64
        return t.sum(axis).astype(F)

    def rms(self, x, n, eps, axis=-1):      # 1 / sqrt(ss / n + eps): f32 scalar arithmetic on the stored sum
        ss = self.sum(x, x, axis)
        return (F(1.0) / np.sqrt(ss / F(n) + F(eps))).astype(F)

    def add_rmsnorm(self, hid, res, w, eps, first, nbo):
        hid, w = np.asarray(hid, F), np.asarray(w, F)
        res = hid.copy() if first else (hid + np.asarray(res, F)).astype(F)
        r = self.rms(res, res.size, eps)
        return ((res * r) * ((w + F(1.0)) if nbo else w)).astype(F), res

    def matvec_q(self, w, sc, bits, q, s):
        wi = unpack(w, bits)
        K, N = wi.shape
        ng = K // 128
        isum = np.matmul(q[:K].reshape(ng, 1, 128).astype(D), wi.reshape(ng, 128, N).astype(D))[:, 0, :]      # |isum| < 2^26: exact
        isf = isum.astype(F)                                                                                    # (float)isum
        comb = (O.bf16_to_f32(np.ascontiguousarray(sc)).reshape(ng, N) * np.asarray(s, F)[:ng, None]).astype(F)
        return self.sum(isf, comb, axis=0)

    def la(self, L, qkvz, ba, eps):
        nk, nv, dk, dv = L["nk"], L["nv"], L["dk"], L["dv"]
        hr = nv // nk; gd = 2 * dk + 2 * dv * hr; kd = nk * dk
        g4 = qkvz.reshape(nk, gd)
        mixed = np.concatenate([g4[:, :dk].reshape(-1), g4[:, dk:2 * dk].reshape(-1), g4[:, 2 * dk:2 * dk + hr * dv].reshape(-1)]).astype(F)
        z = np.ascontiguousarray(g4[:, 2 * dk + hr * dv:]).reshape(nv, dv)
        cs = np.asarray(L["conv_state"], F).reshape(-1, 4)
        cs = np.concatenate([cs[:, 1:], mixed[:, None]], 1)
        co = silu_poly5(self.sum(cs, np.asarray(L["conv_w"], F).reshape(-1, 4), axis=1))

        def l2(src, scale):      # l2norm_expand (decode.rs:3909)
            ss = self.sum(src, src, axis=1)
            inv = np.where(ss > 0, F(1.0) / np.sqrt(np.where(ss > 0, ss, F(1.0))), F(0.0)).astype(F) * F(scale)
            return np.repeat((src * inv[:, None]).astype(F), hr, axis=0)
        q = l2(co[:kd].reshape(nk, dk), L["scale"]); k = l2(co[kd:2 * kd].reshape(nk, dk), 1.0)
        v = co[2 * kd:].reshape(nv, dv)
        b2 = np.asarray(ba, F).reshape(nk, 2, hr)
        beta = sigmoid_libm(b2[:, 0, :].reshape(-1))
        ap = (b2[:, 1, :].reshape(-1) + np.asarray(L["dt_bias"], F)).astype(F)
        sp = np.where(ap > F(20.0), ap, logf(F(1.0) + expf(ap))).astype(F)
        g = (-(expf(L["a_log"])) * sp).astype(F)
        # gated delta rule (decode.rs: la_recurrent): decay, kv = S^T k, delta, S update (one fma per element), o = S^T q
        S = (np.asarray(L["recur_state"], F).reshape(nv, dk, dv) * expf(g)[:, None, None]).astype(F)
        kv = self.sum(S, k[:, :, None], axis=1)
        delta = ((v - kv) * beta[:, None]).astype(F)
        S = (k[:, :, None].astype(D) * delta[:, None, :].astype(D) + S.astype(D)).astype(F)
        o = self.sum(S, q[:, :, None], axis=1)
        r = self.rms(o, dv, eps, axis=1)
        normed = ((o * r[:, None]) * np.asarray(L["norm_w"], F).reshape(nv, dv)).astype(F)
        return (silu_poly5(z) * normed).astype(F).reshape(-1), cs.reshape(-1), S.reshape(-1)

    def gqa(self, L, q_in, k, v, rope, pos, eps, fp8):
        nh, nkv, hd = L["nh"], L["nkv"], L["hd"]
        q2 = np.asarray(q_in, F).reshape(nh, 2, hd)
        q, gate = q2[:, 0, :].copy(), q2[:, 1, :].copy()
        k = np.asarray(k, F).reshape(nkv, hd).copy(); v = np.asarray(v, F).reshape(-1)
        qn = np.asarray(L["q_norm"], F); kn = np.asarray(L["k_norm"], F)
        q = (q * (self.rms(q, hd, eps, axis=1)[:, None] * (qn.reshape(nh, hd) if qn.size == nh * hd else qn[None, :]))).astype(F)
        k = (k * (self.rms(k, hd, eps, axis=1)[:, None] * (kn.reshape(nkv, hd) if kn.size == nkv * hd else kn[None, :]))).astype(F)
        cs, sn = np.asarray(rope[0], F)[pos], np.asarray(rope[1], F)[pos]
        d2 = cs.size
        for b in (q, k):
            x1, x2 = b[:, :d2].copy(), b[:, d2:2 * d2].copy()
            b[:, :d2] = x1 * cs - x2 * sn; b[:, d2:2 * d2] = x2 * cs + x1 * sn
        kc, vc = np.array(L["kv_k"], np.uint16), np.array(L["kv_v"], np.uint16)
        if fp8:
            kc[pos] = O.f32_to_e4m3(k.reshape(-1)); vc[pos] = O.f32_to_e4m3(v)
        else:
            kc[pos] = O.f32_to_f16_bits(k.reshape(-1)); vc[pos] = O.f32_to_f16_bits(v)
        seq = pos + 1; grp = nh // nkv
        kf = cache_to_f32(kc[:seq], fp8).reshape(seq, nkv, hd); vf = cache_to_f32(vc[:seq], fp8).reshape(seq, nkv, hd)
        out = np.empty((nh, hd), F); self.probs = np.empty((nh, seq), F)
        for h in range(nh):
            sc = (self.sum(kf[:, h // grp, :], q[h][None, :], axis=1) * F(L["sm_scale"])).astype(F)
            e = expf(sc - sc.max())
            p = (e * (F(1.0) / self.sum(e))).astype(F)
            self.probs[h] = p
            out[h] = self.sum(p[:, None], vf[:, h // grp, :], axis=0)
        if L["gated"]:
            out = (out * sigmoid_libm(gate)).astype(F)
        return out.reshape(-1), kc, vc

    def route(self, gate, hid, k, scoring, esc):
        lg = self.sum(np.asarray(gate, F), np.asarray(hid, F)[None, :], axis=1)
        if scoring == 1:
            e = expf(lg - lg.max())
            scores = (e * (F(1.0) / self.sum(e))).astype(F)
        else:      # element-wise poly-4 sigmoid: the oracle's own scores
            scores = O.route_score_topk(lg, k, scoring, True, esc)[2]
        sel = (scores + np.asarray(esc, F)).astype(F) if esc is not None else scores
        ids = O.topk_indices(sel, k)
        w = scores[ids]
        s = self.sum(w)
        if s > 0:
            w = (w / s).astype(F)
        return lg, ids, w, sel

    def routed(self, experts, w, act_bf16):
        q, s = O.quant_act_int16_bf16(act_bf16)
        eo = []
        for e in experts:
            gu = self.matvec_q(e.w13, e.w13_scales, e.num_bits, q, s)
            _, hq, hs = O.silu_quant_int16(gu[:e.inter], gu[e.inter:])
            eo.append(self.matvec_q(e.w2, e.w2_scales, e.w2_bits, hq, hs))
        return self.sum(np.asarray(w, F)[:, None], np.stack(eo), axis=0)

    def sig(self, x):
        return sigmoid_libm(x)


def step(orc, token, pos, ops, fp8=False):
    """one decode step of the one-layer model held by the OracleDecode `orc`, from the state in orc.layers[0] (left untouched) -> taps"""
    assert len(orc.layers) == 1
    L = orc.layers[0]; eps, nbo = orc.eps, orc.nbo
    T = {}

    def mv(wid, x):
        w, sc, rows, cols, bits = orc.weights[wid]
        q, s = O.quant_act_int16_f32(np.ascontiguousarray(np.asarray(x, F)[:cols]))
        return ops.matvec_q(w, sc, bits, q, s)
    hid, res = ops.add_rmsnorm(orc.emb[token].copy(), np.zeros(orc.H, F), orc.norms[L["in_norm"]], eps, True, nbo)
    if L["attn"] == "la":
        gated, cs, rs = ops.la(L, mv(L["qkvz"], hid), mv(L["ba"], hid), eps)
        T["conv_new"] = np.asarray(cs, F).reshape(-1, 4)[:, 3].copy(); T["recur"] = np.asarray(rs, F).reshape(L["nv"], -1)
        hid = mv(L["out"], gated)
    else:
        ao, kc, vc = ops.gqa(L, mv(L["q"], hid), mv(L["k"], hid), mv(L["v"], hid), orc.rope, pos, eps, fp8)
        T["k_code"], T["v_code"] = kc[pos].copy(), vc[pos].copy()
        T["k_row"], T["v_row"] = cache_to_f32(kc[pos], fp8), cache_to_f32(vc[pos], fp8)
        hid = mv(L["o"], ao)
    hid, res = ops.add_rmsnorm(hid, res, orc.norms[L["post_norm"]], eps, False, nbo)
    T["resid_attn"] = res
    if L["mlp"] == "moe":
        lg, ids, w, sel = ops.route(L["gate"], hid, orc.topk, orc.scoring, L.get("esc"))
        T["router_logits"], T["router_ids"], T["router_w"] = lg, np.asarray(ids, np.int32), np.asarray(w, F)
        if sel is not None:
            T["router_sel"] = sel
        moe = ops.routed([L["experts"][i] for i in ids], w, O.f32_to_bf16(hid))
        if orc.rsf != F(1.0):
            moe = (moe * orc.rsf).astype(F)
        gu = mv(L["sgu"], hid); si = gu.size // 2
        sh = mv(L["sd"], O.fast_silu_mul(gu[:si], gu[si:]))
        sh = (sh * ops.sig(mv(L["sg"], hid)[0])).astype(F)
        hid = (moe + sh).astype(F)
    else:
        g, u = mv(L["gate_w"], hid), mv(L["up_w"], hid)
        h = np.zeros(orc.weights[L["down_w"]][3], F); h[:g.size] = O.fast_silu_mul(g, u)
        hid = mv(L["down_w"], h)
    T["moe_out"] = hid
    hid, res = ops.add_rmsnorm(hid, res, orc.norms[orc.final_norm], eps, False, nbo)
    T["resid_final"], T["normed"] = res, hid
    T["logits"] = mv(orc.lm_head, hid)
    return T


# ---- the cases of tests/test_decode_stages.py (CPU) and tests/test_decode_fast_stages_gpu.py ----------------------------------------------------------
N_TOK = 6
CAP = 2e-4          # 4 * max(e_exact, e_tree) may not pass a tenth of the whole-model bound of tests/test_decode_fast_gpu.py
GQA_POS = [0, 1, 31, 32, 33, 299]
BASE = (256, 512, 16, 4, 128, 128)      # H, V, E, k, I, SI
UNEVEN = (384, 512, 16, 4, 384, 384)    # three 128-groups on four waves for every matvec of the step


ATTN_TAPS = ("conv_new", "recur", "k_row", "v_row", "resid_attn", "router_logits")
MLP_TAPS = ("router_logits", "router_w", "moe_out", "resid_final", "normed", "logits")


def _c(name, cfg, spikes, **kw):
    return dict(name=name, cfg=cfg, spikes=spikes, taps=ATTN_TAPS, **kw)


def _m(name, cfg, spikes, **kw):
    return dict(name=name, cfg=dict(cfg, out_scale=0.0), spikes=spikes, taps=MLP_TAPS, **kw)


# Two kinds of case.  ATTENTION cases read the taps up to the router logits.  Past that point the reference ALONE breaks the cap on most seeds: the routed experts
# read bf16(hidden), and the 1e-5 that INT16 digit flips of the out projection's input leave in the residual is enough to move a bf16 digit (2^-8 of an element)
# of that vector on every other token -- measured 5e-5 ... 1.4e-3 at moe_out between the oracle and float64.  So the MLP cases isolate the second half of the
# layer the way the one-layer model isolates the layer: the out / o projection's weights are zero (out_scale = 0.0), the attention branch adds exactly nothing
# in every mode, and the post-attention norm, router, experts, combine, final norm and lm_head see bit-identical input.
# Seeds: 48, 49 (gqa-128-f16, gqa-256-f16) and 51 (gqa-128-e4m3) were replaced by 76, 72 and 74.  With 48 / 49 one f16 cache element of the appended row sat on a
# rounding boundary between the oracle's chain and the float64 sum (one f16 step = 2.5e-4 / 2.9e-4 of the row's largest value: past the cap with the reference
# alone; about one seed in two does this); with 51 the scaled K row had a negative score in every head and carried 0.8 % of the probability instead of most of it.
# digit_taps (moe-e130-k6 alone): taps whose bound also admits ONE step of ONE INT16 digit of a routed expert's silu * up image (digit_step below).  On two of
# its six tokens the mode's gate | up sums (K split over two waves) land on the other side of a rounding boundary of that quantiser than both the oracle's
# chain and float64: the difference of the MoE output is one column of the expert's down matrix (cosine 0.9998) on one token and two columns on the other.
# spikes: the element of the embedding rows fed first that holds 90 % of the row's energy: index 0, H - 1, either side of a 64-lane boundary and of a 256-thread
# boundary (H = 384).  hot: cached K row scaled by 16 for the step at position 299 (first row, a 32-position batch boundary, last cached row).
CASES = [
    _c("la-2-4", dict(kinds=["la"], dims=BASE, la_heads=(2, 4), seed=41), (0, 255), eager=True),
    _c("la-1-2", dict(kinds=["la"], dims=BASE, la_heads=(1, 2), seed=42), (63, 64)),
    _c("la-4-16", dict(kinds=["la"], dims=BASE, la_heads=(4, 16), seed=43), (127, 128)),
    _c("la-2-4-hot-head", dict(kinds=["la"], dims=BASE, la_heads=(2, 4), seed=44), (191, 192), hot_head=1),
    _c("uneven-la", dict(kinds=["la"], dims=UNEVEN, seed=45), (255, 256)),
    _c("uneven-gqa", dict(kinds=["gqa"], dims=UNEVEN, hd=128, seed=46), (0, 383)),
    _c("gqa-64-f16", dict(kinds=["gqa"], dims=BASE, kv_max=300, hd=64, seed=47), (63, 64), eager=True, hot=0, two=True),
    _c("gqa-128-f16", dict(kinds=["gqa"], dims=BASE, kv_max=300, hd=128, seed=76), (0, 255), hot=32, two=True),
    _c("gqa-256-f16", dict(kinds=["gqa"], dims=BASE, kv_max=300, hd=256, seed=72), (127, 128), hot=298, two=True),
    _c("gqa-64-e4m3", dict(kinds=["gqa"], dims=BASE, kv_max=300, hd=64, seed=50), (191, 192), hot=298, two=True, fp8=True),
    _c("gqa-128-e4m3", dict(kinds=["gqa"], dims=BASE, kv_max=300, hd=128, seed=74), (63, 64), hot=0, two=True, fp8=True),
    _c("gqa-256-e4m3", dict(kinds=["gqa"], dims=BASE, kv_max=300, hd=256, seed=52), (0, 255), hot=31, two=True, fp8=True),
    _c("wide-2048", dict(kinds=["gqa"], dims=(2048, 512, 16, 10, 512, 512), hd=256, nh=8, seed=53), (2047,), n_tok=1),
    _c("wide-4096", dict(kinds=["gqa"], dims=(4096, 512, 16, 8, 256, 256), hd=128, nh=16, seed=54), (256,), n_tok=1),
    _m("moe-int4", dict(kinds=["la"], dims=BASE, seed=60), (0, 255), lm_two=True),
    _m("moe-int8", dict(kinds=["la"], dims=BASE, wbits=8, seed=55), (63, 64)),
    _m("moe-sigmoid-rsf", dict(kinds=["gqa"], dims=BASE, scoring=0, norm_bias_one=False, rsf=2.5, seed=56), (127, 128)),
    _m("moe-e130-k6", dict(kinds=["gqa"], dims=(256, 512, 130, 6, 128, 128), seed=57), (191, 192), digit_taps=("moe_out", "resid_final")),
    _m("moe-shared-3x", dict(kinds=["la"], dims=(256, 512, 16, 4, 128, 384), seed=58), (0, 255)),
    _m("dense", dict(kinds=["la"], dims=BASE, with_dense=True, seed=59), (63, 64)),
    _m("uneven-mlp", dict(kinds=["la"], dims=UNEVEN, seed=61), (255, 256)),
    _m("wide-2048-mlp", dict(kinds=["la"], dims=(2048, 512, 16, 10, 512, 512), la_heads=(4, 8), seed=62), (2047,), n_tok=1),
    _m("wide-4096-mlp", dict(kinds=["la"], dims=(4096, 512, 16, 8, 256, 256), la_heads=(4, 8), seed=63), (256,), n_tok=1),
]


def tokens(case):
    """(token, position) pairs: the spike rows first, then fixed other rows; GQA short-cache cases walk the batch boundaries of the one-launch form"""
    n = case.get("n_tok", N_TOK)
    toks = ([3 + 5 * i for i in range(len(case["spikes"]))] + [101, 202, 303, 404])[:n]
    pos = GQA_POS if case["cfg"].get("kv_max") == 300 else [5, 6, 7, 8, 9, 10]
    return list(zip(toks, pos[:n]))


def build_case(case, oracle_only=False):
    """tests.test_decode_gpu.build + the case's state edits -> (st, eng, orc, keep, d); the state arrays of d["state"] and of orc.layers[0] are the step's reset state"""
    from tests.test_decode_gpu import build
    _UNPACK.clear()
    toks = [t for t, _ in tokens(case)]
    st, eng, orc, keep, d = build(emb_spikes=tuple(zip(toks, case["spikes"])), oracle_only=oracle_only, **case["cfg"])
    L, S = orc.layers[0], d["state"]
    fp8 = bool(case.get("fp8"))
    if fp8:      # E4M3 codes in place of the f16 words (u8 for the store, u16 slots for the oracle)
        rng = np.random.default_rng(case["cfg"]["seed"])
        S["kv_k"][0] = O.f32_to_e4m3((rng.standard_normal(S["kv_k"][0].shape) * 0.5).astype(F))
        S["kv_v"][0] = O.f32_to_e4m3((rng.standard_normal(S["kv_v"][0].shape) * 0.5).astype(F))
    if "hot" in case:      # a power of two: exact in f16 and in E4M3 (|x| * 16 stays far below both formats' largest value)
        r = case["hot"]
        S["kv_k"][0][r] = O.f32_to_e4m3((e4m3_lut()[S["kv_k"][0][r]] * F(16.0)).astype(F)) if fp8 else O.f32_to_f16_bits(S["kv_k"][0][r].view(np.float16).astype(F) * F(16.0))
    if L["attn"] == "gqa":
        L["kv_k"], L["kv_v"] = S["kv_k"][0].astype(np.uint16), S["kv_v"][0].astype(np.uint16)
    if "hot_head" in case:      # one value head's state 100 x larger: another decay / delta-rule cancellation
        per = d["dk"] * d["dv"]; h = case["hot_head"]
        S["recur"][0][h * per:(h + 1) * per] *= F(100.0)
        L["recur_state"] = S["recur"][0].copy()
    return st, eng, orc, keep, d


def digit_step(orc, token, pos):
    """the largest absolute change of moe_out that ONE step of ONE INT16 digit of a routed expert's silu * up image causes in the
    float64 model: routing weight * rsf * the group's activation scale * the largest |w2| entry (times its scale) of that element's row"""
    L = orc.layers[0]
    ops = Num(False)
    hid, res = ops.add_rmsnorm(orc.emb[token].copy(), np.zeros(orc.H, F), orc.norms[L["in_norm"]], orc.eps, True, orc.nbo)
    t = step(orc, token, pos, ops)
    hid, _ = ops.add_rmsnorm(np.zeros(orc.H, F), t["resid_attn"], orc.norms[L["post_norm"]], orc.eps, False, orc.nbo)      # MLP cases: the branch adds nothing
    q, s = O.quant_act_int16_bf16(O.f32_to_bf16(hid))
    worst = 0.0
    for e, w in zip(t["router_ids"], t["router_w"]):
        ex = L["experts"][e]
        gu = ops.matvec_q(ex.w13, ex.w13_scales, ex.num_bits, q, s)
        _, _, hs = O.silu_quant_int16(gu[:ex.inter], gu[ex.inter:])
        col = np.abs(unpack(ex.w2, ex.w2_bits).astype(D)) * np.repeat(O.bf16_to_f32(np.ascontiguousarray(ex.w2_scales)).astype(D), 128, axis=0)
        worst = max(worst, float((col.max(axis=1) * np.repeat(hs.astype(D), 128)).max() * float(w) * float(orc.rsf)))
    return worst


def rel_err(a, ref):
    """max |a - ref| / max |ref|; 2-D taps (recurrent state: one row per head) are normalised per row, the worst row counts"""
    a, ref = np.asarray(a, D), np.asarray(ref, D)
    if ref.ndim == 2:
        return max(rel_err(x, y) for x, y in zip(a, ref))
    return float(np.abs(a - ref).max() / max(np.abs(ref).max(), 1e-300))


def router_gap_ok(t64, e_exact_logits, k):
    """a token's router ids count only where the float64 model's selection is not a near-tie: (score_k - score_k+1) / max score > 100 * e_exact(router logits)"""
    sel = np.sort(np.asarray(t64["router_sel"], D))[::-1]
    return bool((sel[k - 1] - sel[k]) / np.abs(sel).max() > 100.0 * e_exact_logits)
