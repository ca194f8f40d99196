"""Builds and runs tests/cpp/test_stream_shift.cpp: kz::stream_shift on the host under the address and undefined-behaviour
sanitizers.  A stand-alone program that links the host model code only (kzero_amd/csrc/kz_model.cpp), built the way
tests/test_host_cpp.py builds its programs."""
import os
import subprocess

import pytest

from kzero_amd import synth

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(REPO, "tests", "cpp")
BUILD = os.path.join(CPP, "build")
GOLDEN = os.path.join(REPO, "tests", "golden")


@pytest.mark.timeout(300)
def test_stream_shift_host_code_with_sanitizers(tmp_path):
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "test_stream_shift_asan")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", os.path.join(CPP, "test_stream_shift.cpp"),
                           os.path.join(REPO, "kzero_amd", "csrc", "kz_model.cpp"), "-o", exe])
    models = []
    for name, args, kw in [("chess_2x256", ("chess", 2, 256, "attention"), {"block_gain": 64.0}),
                           ("ataxx7_2x16", ("ataxx-7", 2, 16, "ataxx_conv"), {}),
                           ("go9_3x48", ("go-9", 3, 48, "conv"), {})]:
        path = tmp_path / f"{name}.kzm"
        path.write_bytes(synth.random_model(*args, seed=5, **kw))
        models.append(str(path))
    models.append(os.path.join(GOLDEN, "chess_2x32_dense_h.kzm"))  # a trained-like golden network, another head
    out = subprocess.run([exe, *models], capture_output=True, text=True, timeout=200)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "stream shift tests ok" in out.stdout and out.stdout.count(": checked") == len(models)


def test_cpp_mirror_shift_for_and_model_methods():
    """kzero_amd/csrc/host/hip_network.hpp: shift_for follows the rule's table; HipModel::stream_shift and range_sites go through
    the C ABI (no GPU needed)."""
    os.makedirs(BUILD, exist_ok=True)
    lib = os.path.join(REPO, "kzero_amd")
    exe = os.path.join(BUILD, "test_hip_stream_shift")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-pthread", os.path.join(CPP, "test_hip_stream_shift.cpp"),
                           "-o", exe, f"-L{lib}", "-lkzhip", f"-Wl,-rpath,{lib}"])
    out = subprocess.run([exe, os.path.join(GOLDEN, "ataxx7_4x64.kzm")], capture_output=True, text=True, timeout=100)
    assert out.returncode == 0 and "hip stream shift tests ok" in out.stdout, out.stdout + out.stderr
