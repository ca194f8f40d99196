"""The C++ mirror's half of the per-board status and the range fallback (kzero_amd/csrc/host/hip_network.hpp:
HipNetwork::set_range_fallback, evaluate_batch through kz_engine_wait_decoded_status, the fell_back_boards counter):
tests/cpp/test_hip_board_status.cpp, compiled against the C ABI here and run under -m gpu — wired the way
tests/test_symmetry_average.py wires test_hip_symmetry_average.cpp."""
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
    exe = os.path.join(BUILD, "test_hip_board_status")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-pthread",
                           os.path.join(CPP, "test_hip_board_status.cpp"), "-o", exe, f"-L{LIB}", "-lkzhip", f"-Wl,-rpath,{LIB}"])
    return exe


def test_hip_board_status_test_compiles_against_the_c_abi():
    _build_hip_test()


@pytest.mark.gpu
def test_hip_network_falls_back_and_counts_on_gpu(tmp_path):
    """An Ataxx 3 x 128 network (tower_resident_f16g+heads), 37 boards, three of them out of the f16 range."""
    exe = _build_hip_test()
    path = tmp_path / "ataxx7_3x128.kzm"
    path.write_bytes(synth.random_model("ataxx-7", 3, 128, "ataxx_conv", seed=5))
    out = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "hip board status tests ok" in out.stdout, out.stdout + out.stderr
