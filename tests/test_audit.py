"""The shadow audit (include/kz_hip.h: kz_audit_stats, kz_engine_set_audit, kz_engine_audit_stats), as far as no GPU is needed:
the two entries exist in the header, the built library and capi.py; the struct has the layout the bindings mirror (a C99 program
compiled against the header asserts the size and the offsets); the argument errors that are reached before any HIP call come back
as messages naming the function; and the shim's switch KZ_HIP_AUDIT is the shim's — no file of the library reads it."""
import ctypes as C
import os
import re
import subprocess

from kzero_amd import capi

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(REPO, "include", "kz_hip.h")).read()
HIP_RS = open(os.path.join(REPO, "kzero_amd", "rust", "hip.rs")).read()
HIP_NETWORK = open(os.path.join(REPO, "kzero_amd", "csrc", "host", "hip_network.hpp")).read()

ENTRIES = ("kz_engine_set_audit", "kz_engine_audit_stats")
# (type, name, elements) in the header's order, and the offsets a C compiler must give them
FIELDS = [("int64_t", "batches", 1), ("int64_t", "boards", 1), ("int64_t", "moves", 1), ("int64_t", "skipped", 1),
          ("float", "max_abs_value", 5), ("float", "max_abs_prob", 1), ("double", "sum_sq_value", 5), ("double", "sum_sq_prob", 1)]
OFFSETS = {"batches": 0, "boards": 8, "moves": 16, "skipped": 24, "max_abs_value": 32, "max_abs_prob": 52, "sum_sq_value": 56,
           "sum_sq_prob": 96}
SIZEOF = 104


def test_entries_exist_in_the_header_the_library_and_capi():
    code = re.sub(r"/\*.*?\*/", " ", HEADER, flags=re.S)
    lib = C.CDLL(capi.LIB_PATH)
    for name in ENTRIES:
        assert re.search(rf"\bint {name}\s*\(", code), f"{name} is not declared in kz_hip.h"
        assert hasattr(lib, name), f"{name} is not exported by the built library"
        assert name in capi.SIGNATURES
    assert re.search(r"int kz_engine_set_audit\(kz_engine \*engine, int dtype, int period, int boards\);", code)
    assert re.search(r"int kz_engine_audit_stats\(kz_engine \*engine, void \*out, int reset\);", code)
    for method in ("set_audit", "audit_stats"):
        assert callable(getattr(capi.Engine, method))
    # the C++ mirror and the Rust shim go through both
    for name in ENTRIES:
        assert f"{name}(" in HIP_NETWORK
        externs = re.search(r'extern "C" \{(.*?)\n\}', HIP_RS, flags=re.S).group(1)
        assert re.search(rf"\bfn {name}\s*\(", externs) and re.search(rf"\b{name}\(", HIP_RS.replace(externs, ""))


def test_struct_fields_match_in_header_capi_and_rust():
    code = re.sub(r"/\*.*?\*/", " ", HEADER, flags=re.S)
    body = re.search(r"typedef struct kz_audit_stats \{(.*?)\} kz_audit_stats;", code, flags=re.S).group(1)
    c_fields = [(t, n, int(k) if k else 1) for t, n, k in re.findall(r"(int64_t|float|double)\s+(\w+)(?:\[(\d+)\])?;", body)]
    assert c_fields == FIELDS
    ctypes_of = {"int64_t": C.c_int64, "float": C.c_float, "double": C.c_double}
    assert [(n, ctypes_of[t] * k if k > 1 else ctypes_of[t]) for t, n, k in FIELDS] == list(capi.AuditStats._fields_)
    assert C.sizeof(capi.AuditStats) == SIZEOF
    for name, offset in OFFSETS.items():
        assert getattr(capi.AuditStats, name).offset == offset, name
    r_struct = re.search(r"pub struct KzAuditStats \{(.*?)\}", HIP_RS, flags=re.S).group(1)
    rust_of = {"int64_t": "i64", "float": "f32", "double": "f64"}
    assert re.findall(r"pub (\w+): ([^,]+),", r_struct) == [(n, f"[{rust_of[t]}; {k}]" if k > 1 else rust_of[t]) for t, n, k in FIELDS]
    assert "#[repr(C)]" in HIP_RS.split("pub struct KzAuditStats")[0][-80:]


def test_a_c99_program_sees_the_documented_layout(tmp_path):
    """Compiled the way tests/test_abi.py::test_header_is_plain_c_and_the_c_example_links compiles against the header."""
    checks = " && ".join([f"sizeof(kz_audit_stats) == {SIZEOF}"] + [f"offsetof(kz_audit_stats, {n}) == {o}" for n, o in OFFSETS.items()])
    src = tmp_path / "audit_layout.c"
    src.write_text('#include <stddef.h>\n#include "kz_hip.h"\n'
                   "int main(void) {\n"
                   "    int (*set_audit)(kz_engine *, int, int, int) = kz_engine_set_audit;\n"
                   "    int (*audit_stats)(kz_engine *, void *, int) = kz_engine_audit_stats;\n"
                   "    kz_audit_stats st;\n"
                   "    if (set_audit(NULL, KZ_DTYPE_F32, 1, 1) == 0 || audit_stats(NULL, &st, 0) == 0) return 2;\n"
                   f"    return {checks} ? 0 : 1;\n"
                   "}\n")
    lib = os.path.join(REPO, "kzero_amd")
    exe = tmp_path / "audit_layout"
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(REPO, "include"), str(src),
                           "-L", lib, "-lkzhip", f"-Wl,-rpath,{lib}", "-o", str(exe)])
    assert subprocess.run([str(exe)]).returncode == 0


def test_argument_errors_that_need_no_gpu():
    lib = capi.load()
    raw = capi.AuditStats()
    for dtype in (capi.KZ_DTYPE_F32, capi.KZ_DTYPE_F32_SPLIT16, -1, 7):
        assert lib.kz_engine_set_audit(None, dtype, 1, 1) != 0
        assert lib.kz_last_error().decode() == "kz_engine_set_audit: null engine"
    assert lib.kz_engine_audit_stats(None, C.byref(raw), 0) != 0
    assert lib.kz_last_error().decode() == "kz_engine_audit_stats: null engine"
    # (a null `out` on an engine needs a GPU: tests/test_gpu_audit.py has it; a null engine is looked at first)
    assert lib.kz_engine_audit_stats(None, None, 1) != 0
    assert lib.kz_last_error().decode().startswith("kz_engine_audit_stats: null")


def test_derived_root_mean_squares():
    raw = capi.AuditStats()
    assert capi.AuditResult(raw).rms_prob == 0.0 and not capi.AuditResult(raw).rms_value.any()
    raw.boards, raw.moves, raw.sum_sq_prob = 4, 8, 2.0
    for c in range(5):
        raw.sum_sq_value[c] = float(c)
    r = capi.AuditResult(raw)
    assert r.rms_prob == 0.5 and r.rms_value.tolist() == [(c / 4) ** 0.5 for c in range(5)]
    assert r.max_abs_value.dtype.name == "float32" and r.max_abs_value.shape == (5,) and r.sum_sq_value.dtype.name == "float64"


def test_the_switch_is_the_shims_and_the_library_reads_nothing_new():
    assert 'std::env::var("KZ_HIP_AUDIT")' in HIP_RS
    csrc = os.path.join(REPO, "kzero_amd", "csrc")
    for root, dirs, files in os.walk(csrc):
        dirs[:] = [d for d in dirs if not d.startswith("build")]
        for name in files:
            if name.endswith((".hip", ".hpp", ".cpp", ".h", ".sh")):
                assert "KZ_HIP_AUDIT" not in open(os.path.join(root, name)).read(), os.path.join(root, name)
    block = HEADER[HEADER.index("Environment switches read by kz_engine_create"):HEADER.index("Name of the path the engine chose")]
    assert "KZ_HIP_AUDIT" not in block
    # the library's strings: the messages of the two entries name dtypes only, no other KZ_ token (tests/test_abi.py holds the set)
    out = subprocess.run(["strings", "-n", "4", capi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    mine = [ln for ln in out.splitlines() if "kz_engine_set_audit" in ln or "kz_engine_audit_stats" in ln]
    assert mine
    for ln in mine:
        assert set(re.findall(r"\bKZ_[A-Z0-9_]+\b", ln)) <= {"KZ_DTYPE_F32", "KZ_DTYPE_F16", "KZ_DTYPE_F32_SPLIT16"}, ln
