"""Builds and runs tests/cpp/test_tower_boundary.cpp: conv A's epilogue of the chess f16 tower converts to f16 first and
takes the ReLU on the packed f16 bits (kzero_amd/csrc/kz_tower_boundary.hpp).  The program holds that order to the bits of
ReLU-then-convert for every f16 value and rounding boundary with their f32 neighbours, the f32 corner patterns (zeros,
subnormals, the overflow threshold, infinities, NaNs of both signs) and 40 million random f32 bit patterns.  A host build of
the header's own functions by the HIP compiler's clang (the header uses its vector types and _Float16); no GPU needed."""
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(REPO, "tests", "cpp")
BUILD = os.path.join(CPP, "build")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.mark.timeout(300)
def test_convert_then_packed_relu_equals_relu_then_convert():
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "test_tower_boundary")
    subprocess.check_call([HIPCC, "-x", "c++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-fsanitize=undefined",
                           "-fno-sanitize-recover=undefined", os.path.join(CPP, "test_tower_boundary.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=200)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "tower boundary relu tests ok" in out.stdout and " 0 mismatches" in out.stdout
