#!/usr/bin/env python3
"""Recorded behaviour of the reference's paged-KV bookkeeping classes (python/krasis/kv_cache.py:38-272: PagedKVCache, SequenceKVState) for
tests/test_kv_cache.py::test_side_by_side_with_the_reference_classes.

    python tests/golden/make_golden_kv_cache.py <reference checkout>     # writes tests/golden/kv_cache_paging.npz

Imported from where it lies (nothing is copied); only its results are stored.  Three pools of 48 pages over 2 layers with FP16 pages -- GQA, split MLA,
combined MLA -- each driven through the same allocation sequence (ensure_capacity + advance of 1, 15, 1, 40, 100 tokens).  Recorded after every step: the
page list, seq_len, last_page_len, free_page_count, max_context_tokens, kv_indices and block_tables; for the combined store the whole cache after
store_kv_combined of rows that are a fixed integer pattern (exact in FP16); the message of the exhaustion error; the free count after free().
"""
import os
import sys
import types

import numpy as np
import torch

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "kv_cache_paging.npz")
STEPS = (1, 15, 1, 40, 100)
CONFIGS = ((False, False), (True, False), (True, True))          # (mla, combined)


class Cfg:
    def __init__(self, mla):
        self.attention_type = "mla" if mla else "gqa"
        self.is_mla, self.is_gqa = mla, not mla
        self.kv_lora_rank, self.qk_rope_head_dim = 512, 64
        self.num_key_value_heads, self.gqa_head_dim = 2, 256


def pattern_rows(n, dim=576):
    """rows whose values are distinct small integers / 8: exact in FP16, the same on every machine"""
    return (((torch.arange(n * dim, dtype=torch.int64) % 2039) - 1019).to(torch.float32) / 8).reshape(n, dim).to(torch.float16)


def import_reference_kv_cache(ref_root):
    src = os.path.join(ref_root, "python", "krasis")
    sys.modules.setdefault("krasis", types.ModuleType("krasis")).__path__ = [src]
    cfgmod = types.ModuleType("krasis.config"); cfgmod.ModelConfig = object; sys.modules["krasis.config"] = cfgmod
    import importlib.util
    spec = importlib.util.spec_from_file_location("krasis.kv_cache", os.path.join(src, "kv_cache.py"))
    mod = importlib.util.module_from_spec(spec); spec.loader.exec_module(mod)
    return mod


def record(ref):
    out = {"steps": np.array(STEPS, np.int64), "configs": np.array(CONFIGS, np.int64)}
    for c, (mla, combined) in enumerate(CONFIGS):
        a = ref.PagedKVCache(Cfg(mla), 2, torch.device("cpu"), max_pages=48, kv_dtype=torch.float16, combined=combined)
        s = ref.SequenceKVState(a)
        scalars = []
        for j, step in enumerate(STEPS):
            s.ensure_capacity(step); s.advance(step)
            scalars.append([s.seq_len, s.last_page_len(), a.free_page_count, a.max_context_tokens])
            out["c%d_s%d_pages" % (c, j)] = np.array(s.pages, np.int64)
            out["c%d_s%d_kv_indices" % (c, j)] = s.kv_indices("cpu").numpy().astype(np.int64)
            out["c%d_s%d_block_tables" % (c, j)] = s.block_tables("cpu").numpy().astype(np.int64)
        out["c%d_scalars" % c] = np.array(scalars, np.int64)
        if combined:
            rows = pattern_rows(s.seq_len)
            s.store_kv_combined(1, rows, torch.arange(s.seq_len))
            out["c%d_kv_cache" % c] = a.kv_cache.view(torch.int16).numpy().view(np.uint16)
        try:
            s.ensure_capacity(10_000)
            raise SystemExit("the reference did not refuse 10 000 tokens")
        except RuntimeError as ex:
            out["c%d_exhausted" % c] = np.array(str(ex))
        s.free()
        out["c%d_free_after" % c] = np.array(a.free_page_count, np.int64)
    return out


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit("usage: make_golden_kv_cache.py <reference checkout>")
    np.savez_compressed(OUT, **record(import_reference_kv_cache(sys.argv[1])))
    print("wrote", OUT, os.path.getsize(OUT), "bytes")
