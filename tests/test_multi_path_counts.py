"""No-GPU checks of kr_decode_multi_path_counts (docs/design/32-multi-pass-plan.md): the Python wrapper names the header's KR_MPC_* counters in the header's
order, and a null store is an error, not a crash.  What the counters say on a GPU is held by
tests/test_multi_options_random_gpu.py and the per-option files."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _read(*parts):
    return open(os.path.join(ROOT, *parts)).read()


def test_the_wrapper_names_the_headers_counters_in_order():
    from krasis_amd.decode_store import CpuDecodeStore
    enum = re.search(r"enum \{\s*KR_MPC_PASSES = 0,(.*?)KR_MPC_COUNT\s*\};", _read("include", "krasis_hip.h"), re.S)
    assert enum, "the KR_MPC_* enum of include/krasis_hip.h"
    names = ["passes"] + [n.lower() for n in re.findall(r"KR_MPC_([A-Z0-9_]+),", re.sub(r"/\*.*?\*/", "", enum.group(1), flags=re.S))]
    assert tuple(names) == CpuDecodeStore.MULTI_PATH_COUNTS


def test_a_null_store_is_a_value_error():
    from krasis_amd import _lib
    lib = _lib.load_library()
    assert lib.kr_decode_multi_path_counts(None, None, 0, 0) == 2      # KR_ERR_VALUE
    assert b"kr_decode_multi_path_counts" in lib.kr_last_error()
