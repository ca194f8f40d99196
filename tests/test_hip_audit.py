"""The C++ mirror's half of the shadow audit (kzero_amd/csrc/host/hip_network.hpp: HipNetwork::set_audit, audit_stats):
tests/cpp/test_hip_audit.cpp, compiled against the C ABI here and run under -m gpu — wired the way
tests/test_hip_board_status.py wires test_hip_board_status.cpp."""
import os
import subprocess

import pytest

from kzero_amd import synth

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(REPO, "tests", "cpp")
BUILD = os.path.join(CPP, "build")
LIB = os.path.join(REPO, "kzero_amd")


def _build_hip_test():
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "test_hip_audit")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-pthread",
                           os.path.join(CPP, "test_hip_audit.cpp"), "-o", exe, f"-L{LIB}", "-lkzhip", f"-Wl,-rpath,{LIB}"])
    return exe


def test_hip_audit_test_compiles_against_the_c_abi():
    _build_hip_test()


@pytest.mark.gpu
def test_hip_network_audits_and_changes_nothing_on_gpu(tmp_path):
    """An Ataxx 3 x 128 network (tower_resident_f16g+heads) in f16, audited against exact f32: two batches of 21 boards."""
    exe = _build_hip_test()
    path = tmp_path / "ataxx7_3x128.kzm"
    path.write_bytes(synth.random_model("ataxx-7", 3, 128, "ataxx_conv", seed=5))
    out = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "hip audit tests ok" in out.stdout, out.stdout + out.stderr
