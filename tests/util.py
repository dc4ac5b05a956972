"""Shared helpers for the GPU parity tests (the oracle is the checker, never the thing measured)."""
import numpy as np

from oracle import oracle as O


def rand_bf16(rng, shape, scale=1.0):
    return O.f32_to_bf16((rng.standard_normal(shape) * scale).astype(np.float32))


def make_experts(rng, E, H, I, bits=4, w2_bits=None, scale=0.05):
    out = []
    for _ in range(E):
        g = rand_bf16(rng, (I, H), scale); u = rand_bf16(rng, (I, H), scale); d = rand_bf16(rng, (H, I), scale)
        out.append(O.unified_from_bf16(g, u, d, 128, bits, w2_bits))
    return out


def upload(engine, layer, experts, shared=None):
    for e, ex in enumerate(experts):
        engine.load_unified_expert(layer, e, ex.w13, ex.w13_scales, ex.w2, ex.w2_scales, ex.num_bits, ex.w2_bits)
    if shared is not None:
        engine.load_unified_expert(layer, -1, shared.w13, shared.w13_scales, shared.w2, shared.w2_scales, shared.num_bits, shared.w2_bits)


# ---- the recorded refusals of the slot options (tests/golden/slot_option_refusals.json, docs/design/39-slot-option-rules.md) ----------------------------
# the eleven opt-in forms of the batched pass over device slots: the two GQA flash-decode options, then the nine of the rule list in its order
FLAGS = ("multi_attn_fast", "multi_attn_fast_paged", "multi_mla_fast", "multi_extend_mla_flash", "multi_extend_flash", "multi_extend_la_chunk",
         "multi_extend_exact_mfma", "multi_extend_mla_exact_mfma", "multi_attn_exact_split", "multi_mla_exact_split", "multi_extend_la_exact")


def refusal_case(flags, mode=False):
    """the fixture's name of a case: the options that are set, in FLAGS order, and whether the attention-mode bit is"""
    flags = sorted(flags, key=FLAGS.index)
    return ("mode:" if mode else "") + ("all" if len(flags) == len(FLAGS) else "+".join(flags) or "none")


def slot_option_refusals():
    import json
    import os
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "slot_option_refusals.json")) as f:
        return json.load(f)


def recorded_refusal(store, *flags, mode=False):
    """what one step_multi gave on that store ("la/flat", "mla/paged", ...) under those options when the fixture was recorded: "ok", or "<exception type>:
    <message>".  A case the fixture does not hold is a KeyError: the tests that cite a case thereby assert that it exists"""
    fx = slot_option_refusals()
    return fx["messages"][fx["stores"][store][refusal_case(flags, mode)]]


def _csrc(name):
    import os
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "krasis_amd", "csrc", name)) as f:
        return f.read()


def option_field(opt):
    """a slot option is known everywhere: kr_decode_set_option's strcmp line sets its ONE field of the options struct (kr_multi_opts.h), which the store holds
    as one member and the pass hands to the plan in one assignment.  -> the field's name"""
    import re
    field = opt[len("multi_"):]
    assert len(re.findall(r'\n    int %s = \d+; +// "%s"' % (field, opt), _csrc("kr_multi_opts.h"))) == 1, opt
    dec = _csrc("kr_decode.cpp")
    assert dec.count('!strcmp(name, "%s")' % opt) == 1 and "s->mopt.%s = value" % field in dec[dec.index('!strcmp(name, "%s")' % opt):][:600], opt
    assert _csrc("kr_decode_internal.h").count("KrMultiOpts mopt;") == 1 and "opt_" + opt not in _csrc("kr_decode_internal.h")
    pre = _csrc("kr_decode_prefill.cpp")
    assert "o.opt = s->mopt;" in pre[pre.index("int kr_multi_pass("):] and "KrMultiOpts opt;" in _csrc("kr_multi_plan.h")
    return field


def rule_row(opt):
    """the option's row of the ordered rule list (kr_decode_prefill.cpp), up to the next row"""
    import re
    pre = _csrc("kr_decode_prefill.cpp")
    table = pre[pre.index("static const KrOptRule kr_opt_rules[] = {"):pre.index("int kr_option_rules(")]
    rows = re.split(r'\n    (?=\{"multi_)', table)[1:]
    mine = [r for r in rows if r.startswith('{"%s", &KrMultiOpts::%s,' % (opt, opt[len("multi_"):]))]
    assert len(mine) == 1, opt
    return re.sub(r"(\n\s*//[^\n]*)+\s*$", "", mine[0].replace("\n};", ""))      # without the next row's comment or the table's end


def rule_place_seen(opt):
    """the place of an option's rule in the ordered list, where a caller sees it (the recorded cases): behind the attention-mode bit on every main store; standing
    back for the entry point's paged refusal under "multi_attn_fast" alone ("multi_mla_fast" apart); and against every other rule of the list, on each
    single-kind store that refuses both alone in their own words, the pair gives the words of the one that stands earlier.  -> the pairs that were seen"""
    seen = 0
    for other in FLAGS[2:]:
        if other == opt:
            continue
        shown = 0
        for store in ("la/flat", "gqa/flat", "mla/flat", "la/paged", "gqa/paged", "mla/paged"):
            a, b = recorded_refusal(store, opt), recorded_refusal(store, other)
            if '"%s" option covers' % opt in a and '"%s" option covers' % other in b:
                assert recorded_refusal(store, opt, other) == (a if FLAGS.index(opt) < FLAGS.index(other) else b), (store, opt, other)
                shown += 1
        assert shown, (opt, other)
        seen += shown
    for store in ("la", "gqa", "mla", "hybrid"):
        for layout in ("flat", "paged"):
            assert "the attention mode has tolerance bits set (1)" in recorded_refusal("%s/%s" % (store, layout), opt, mode=True)
        if opt != "multi_mla_fast" and store != "mla":      # an MLA store: the GQA options' own MLA clause speaks ahead of the paged refusal
            assert recorded_refusal(store + "/paged", "multi_attn_fast", opt).startswith('RuntimeError: "multi_attn_fast" does not read paged slots'), (store, opt)
    return seen
