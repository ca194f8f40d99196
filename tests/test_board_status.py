"""Per-board status and the range fallback, as far as no GPU is needed: the three entries exist in the built library and in
capi.py, the header, capi.py and the Rust shim agree on their names and on the KZ_BOARD_* constants (a text check in the style of
tests/test_rust_shim_text.py), and the argument errors that are reached before any HIP call come back as messages."""
import ctypes as C
import os
import re

from kzero_amd import capi

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(REPO, "include", "kz_hip.h")).read()
HIP_RS = open(os.path.join(REPO, "kzero_amd", "rust", "hip.rs")).read()
HIP_NETWORK = open(os.path.join(REPO, "kzero_amd", "csrc", "host", "hip_network.hpp")).read()

ENTRIES = ("kz_engine_wait_decoded_status", "kz_engine_eval_packed_decoded_status", "kz_engine_set_range_fallback")
CONSTANTS = {"KZ_BOARD_OK": 0, "KZ_BOARD_BAD_DECODE": 1, "KZ_BOARD_NONFINITE": 2, "KZ_BOARD_FELL_BACK": 4}


def test_entries_exist_in_the_library_and_in_capi():
    lib = C.CDLL(capi.LIB_PATH)
    for name in ENTRIES:
        assert hasattr(lib, name), f"{name} is not exported by the built library"
        assert name in capi.SIGNATURES
    for method in ("wait_decoded_status", "eval_packed_decoded_status", "set_range_fallback"):
        assert callable(getattr(capi.Engine, method))


def test_header_capi_and_rust_shim_agree_on_names_and_constants():
    code = re.sub(r"/\*.*?\*/", " ", HEADER, flags=re.S)
    rust_externs = re.search(r'extern "C" \{(.*?)\n\}', HIP_RS, flags=re.S).group(1)
    for name in ENTRIES:
        assert re.search(rf"\bint {name}\s*\(", code), f"{name} is not declared in kz_hip.h"
        assert re.search(rf"\bfn {name}\s*\(", rust_externs), f"{name} is not bound in hip.rs"
    for name in ("kz_engine_wait_decoded_status", "kz_engine_set_range_fallback"):  # what the shim's logic goes through
        assert re.search(rf"\b{name}\(", HIP_RS.replace(rust_externs, "")), f"hip.rs binds {name} but never calls it"
    for name, value in CONSTANTS.items():
        assert int(re.search(rf"#define {name} (\d+)", HEADER).group(1)) == value
        assert getattr(capi, name) == value
        assert int(re.search(rf"pub const {name}: u8 = (\d+);", HIP_RS).group(1)) == value
    # the status is a bit set: the three error bits are distinct powers of two
    bits = [v for v in CONSTANTS.values() if v]
    assert all(v & (v - 1) == 0 for v in bits) and len(set(bits)) == 3
    # the C++ mirror goes through the status entry and the fallback switch
    assert "kz_engine_wait_decoded_status(" in HIP_NETWORK and "kz_engine_set_range_fallback(" in HIP_NETWORK
    # the shim's switch is the shim's: read in hip.rs, unknown to the library's header list of switches
    assert 'std::env::var("KZ_HIP_RANGE_FALLBACK")' in HIP_RS
    block = HEADER[HEADER.index("Environment switches read by kz_engine_create"):HEADER.index("Name of the path the engine chose")]
    assert "KZ_HIP_RANGE_FALLBACK" not in block


def test_argument_errors_that_need_no_gpu():
    lib = capi.load()
    v, p, s = C.c_void_p(), C.c_void_p(), C.c_void_p()
    for dtype in (capi.KZ_DTYPE_F32, -1, 7):
        assert lib.kz_engine_set_range_fallback(None, dtype) != 0
        assert lib.kz_last_error().decode() == "kz_engine_set_range_fallback: null engine"
    assert lib.kz_engine_wait_decoded_status(None, 0, C.byref(v), C.byref(p), C.byref(s)) != 0
    assert lib.kz_last_error().decode() == "kz_engine_wait_decoded_status: null engine"
    assert lib.kz_engine_wait_decoded_status(None, 0, C.byref(v), C.byref(p), None) != 0
    assert lib.kz_last_error().decode() == "kz_engine_wait_decoded_status: null output"
    assert lib.kz_engine_eval_packed_decoded_status(None, None, 0, None, 1, None, None, None, None, None, None) != 0
    assert "kz_engine_eval_packed_decoded_status: null engine" in lib.kz_last_error().decode()
