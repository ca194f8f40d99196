"""KZ_HIP_STREAM_SHIFT=auto and the two new entries in the three bindings, as text (no cargo in the build image: hip.rs is held to
the header the way tests/test_rust_shim_text.py holds it).  No GPU."""
import os
import re

from kzero_amd import capi

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIP_RS = open(os.path.join(REPO, "kzero_amd", "rust", "hip.rs")).read()
SERVER_RS = open(os.path.join(REPO, "kzero_amd", "rust", "server_hip.rs")).read()
HEADER = open(os.path.join(REPO, "include", "kz_hip.h")).read()
HPP = open(os.path.join(REPO, "kzero_amd", "csrc", "host", "hip_network.hpp")).read()

NEW = ("kz_model_range_profile_fast", "kz_model_range_profile_fast_path")


def header_args(name):
    """The parameter list of a prototype of the header: [(type without spaces, name)]."""
    m = re.search(r"^int " + name + r"\(([^;]*)\);", HEADER, flags=re.M | re.S)
    assert m, name
    out = []
    for p in m.group(1).replace("\n", " ").split(","):
        ty, nm = re.match(r"\s*(.*?)(\w+)\s*$", p).groups()
        out.append((ty.replace(" ", ""), nm))
    return out


def function_body(text, signature):
    """The text of a Rust item from `signature` to the closing brace at its indentation."""
    start = text.index(signature)
    indent = re.search(r"^[ ]*", text[text.rfind("\n", 0, start) + 1:]).group(0)
    end = text.index("\n" + indent + "}\n", start)
    return text[start:end]


def test_hip_rs_parses_auto_and_auto_with_headroom():
    body = function_body(HIP_RS, "impl StreamShift {")
    assert 'v == "auto"' in body and "StreamShift::Auto(2)" in body  # two bits by default
    assert 'strip_prefix("auto:")' in body and re.search(r"StreamShift::Auto\(bits\.parse::<i32>\(\)", body)
    assert "auto[:<headroom bits>]" in body  # the panic's usage line
    env = function_body(HIP_RS, "pub fn stream_shift_from_env(self) -> HipModel {")
    assert "StreamShift::from_env()" in env and "StreamShift::Auto(headroom_bits)" in env
    assert "self.auto_stream_shift(position_sample(), headroom_bits)" in env
    # the sample is process-wide and every HipNetwork feeds it while `auto` is set
    assert "static SAMPLE: OnceLock<PositionSample>" in HIP_RS
    assert "position_sample().offer(device, &self.bits, bits_bytes, &self.scalars_in" in function_body(HIP_RS, "fn prepare(&mut self")
    assert re.search(r"sample_from: match StreamShift::from_env\(\) \{\s*StreamShift::Auto\(_\) => Some\(device\)", HIP_RS)
    # read where it was read before: load_graph
    assert ".stream_shift_from_env()" in function_body(SERVER_RS, "    fn load_graph(&self, path: &str, mapper: M, _: &StartupSettings) -> HipModel {")
    assert "auto[:<headroom bits>]" in SERVER_RS
    # the profile is the fast one, the rule is shift_for, +inf is refused, an empty sample is k = 0
    auto = function_body(HIP_RS, "pub fn auto_stream_shift(&self")
    assert "self.range_profile_fast(" in auto and "shift_for(max_abs, headroom_bits)" in auto
    assert "max_abs.is_finite()" in auto and "return (None, 0, 0.0, 0);" in auto


def test_hip_rs_still_parses_integers():
    body = function_body(HIP_RS, "impl StreamShift {")
    assert "StreamShift::Fixed(v.parse::<i32>()" in body
    assert "Err(_) => StreamShift::Fixed(0)" in body  # unset: the network as trained
    env = function_body(HIP_RS, "pub fn stream_shift_from_env(self) -> HipModel {")
    assert "StreamShift::Fixed(0) => self," in env and "StreamShift::Fixed(k) => self.stream_shift(k)," in env
    assert "[-24, 24]" in body


RUST_TYPES = {"constkz_model*": "*const c_void", "int": "c_int", "constuint8_t*": "*const u8", "size_t": "usize",
              "constfloat*": "*const f32", "float*": "*mut f32", "char*": "*mut c_char"}
CTYPES = {"constkz_model*": capi.C.c_void_p, "int": capi.C.c_int, "constuint8_t*": capi.C.c_void_p, "size_t": capi.C.c_size_t,
          "constfloat*": capi.C.c_void_p, "float*": capi.C.c_void_p, "char*": capi.C.c_char_p}


def test_the_three_bindings_declare_the_new_entries_with_the_headers_argument_lists():
    for name in NEW:
        args = header_args(name)
        # hip.rs: same names, same order, the matching types
        m = re.search(r"fn " + name + r"\(([^)]*)\) -> c_int;", HIP_RS)
        assert m, name
        rust = [tuple(s.strip() for s in p.split(":")) for p in m.group(1).split(",")]
        assert rust == [(nm, RUST_TYPES[ty]) for ty, nm in args], (name, rust)
        # capi.py
        restype, argtypes = capi.SIGNATURES[name]
        assert restype is capi.C.c_int and argtypes == [CTYPES[ty] for ty, _ in args], name
        # the C++ mirror calls it with as many arguments
        call = re.search(name + r"\(ptr_((?:, [^,()]+(?:\(\))?)*)\)\)", HPP)
        assert call and call.group(1).count(",") == len(args) - 1, name
    assert header_args("kz_model_range_profile_fast") == header_args("kz_model_range_profile")
    assert [ty for ty, _ in header_args("kz_model_range_profile_fast_path")] == ["constkz_model*", "char*", "size_t"]
    for method in ("def range_profile_fast(self", "def range_profile_fast_path(self", "def auto_stream_shift(model"):
        assert method in open(os.path.join(REPO, "kzero_amd", "capi.py")).read()
    for method in ("pub fn range_profile_fast(&self", "pub fn range_profile_fast_path(&self", "pub fn auto_stream_shift(&self"):
        assert method in HIP_RS
    for method in ("RangeProfile range_profile_fast(", "std::string range_profile_fast_path()", "AutoShift auto_stream_shift("):
        assert method in HPP


def test_capi_auto_stream_shift_without_boards_measures_nothing():
    import numpy as np
    from kzero_amd import synth
    model = capi.Model(blob=synth.random_model("ataxx-7", 2, 128, "ataxx_conv", seed=5))
    same, k, m, boards = capi.auto_stream_shift(model, 0, np.zeros((0, model.info.bits_bytes), np.uint8), np.zeros((0, 1), np.float32))
    assert same is model and (k, m, boards) == (0, 0.0, 0)
    assert model.range_profile_fast_path() == "tower_resident_f32"
    assert capi.Model(blob=synth.random_model("go-19", 2, 64, "conv", seed=5)).range_profile_fast_path() == "conv_igemm_f32"
