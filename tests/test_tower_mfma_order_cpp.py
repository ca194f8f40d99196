"""Builds and runs tests/cpp/test_tower_mfma_order.cpp: the order in which a k-step of the chess f16 tower issues its MFMAs
(kzero_amd/csrc/kz_tower_mfma_order.hpp) visits every accumulator of the k-step's tile range exactly once, changes exactly
one operand register from one MFMA to the next, keeps the B register over a dy seam where the next range has it, and never
returns to an accumulator within four positions.  A host build of the header the kernel includes; no GPU needed."""
import os
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(REPO, "tests", "cpp")
BUILD = os.path.join(CPP, "build")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.mark.timeout(120)
def test_mfma_order_table():
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "test_tower_mfma_order")
    subprocess.check_call([HIPCC, "-x", "c++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-fsanitize=undefined",
                           "-fno-sanitize-recover=undefined", os.path.join(CPP, "test_tower_mfma_order.cpp"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    print(out.stdout)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "tower mfma order tests ok, 0 failures" in out.stdout
