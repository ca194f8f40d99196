"""The shim chooses the stream shift (kzero_amd/csrc/host/position_sample.hpp: PositionSample; hip_network.hpp:
HipNetwork::set_position_sample, HipModel::range_profile_fast / auto_stream_shift, StreamShiftEnv): tests/cpp/test_hip_auto_shift.cpp,
compiled against the C ABI here — its CPU half (the sample's ring and prefix rule, two offering threads, the parser) runs without a
GPU, the whole of it under -m gpu — wired the way tests/test_hip_audit.py wires test_hip_audit.cpp."""
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
    exe = os.path.join(BUILD, "test_hip_auto_shift")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-pthread",
                           os.path.join(CPP, "test_hip_auto_shift.cpp"), "-o", exe, f"-L{LIB}", "-lkzhip", f"-Wl,-rpath,{LIB}"])
    return exe


def test_hip_auto_shift_test_compiles_and_its_cpu_half_passes():
    exe = _build_hip_test()
    out = subprocess.run([exe, "--cpu"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "hip auto shift tests ok" in out.stdout, out.stdout + out.stderr


@pytest.mark.gpu
def test_hip_network_samples_and_the_model_shifts_itself_on_gpu(tmp_path):
    """An Ataxx 2 x 128 network A and B = A on a stream 2^18 times as large: three f16 batches of 21 boards feed the sample, B's
    profile on the sampled boards is past 65504 everywhere, the shifted B in f16 is A in exact f32 within the decoded f16 contract."""
    exe = _build_hip_test()
    path = tmp_path / "ataxx7_2x128.kzm"
    path.write_bytes(synth.random_model("ataxx-7", 2, 128, "ataxx_conv", seed=5))
    out = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120)
    print(out.stdout)
    assert out.returncode == 0 and "hip auto shift tests ok" in out.stdout, out.stdout + out.stderr
