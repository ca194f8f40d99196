"""Every board under every symmetry, averaged inside the engine (the `_avg` entries of include/kz_hip.h), the parts that need
no GPU: the entries in the built library, the numpy statement of the averaging that tests/test_gpu_symmetry_average.py holds
the kernels to, and the C++ mirror's test compiling against the C ABI.  The GPU half of that mirror
(HipNetwork::set_average_symmetries against the AverageSymmetryNetwork wrapper) is tests/cpp/test_hip_symmetry_average.cpp,
run here under -m gpu."""
import os
import subprocess

import numpy as np
import pytest

from kzero_amd import capi

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(REPO, "tests", "cpp")
BUILD = os.path.join(CPP, "build")
GOLDEN = os.path.join(REPO, "tests", "golden")
LIB = os.path.join(REPO, "kzero_amd")


def _build_hip_test():
    os.makedirs(BUILD, exist_ok=True)
    exe = os.path.join(BUILD, "test_hip_symmetry_average")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-pthread",
                           os.path.join(CPP, "test_hip_symmetry_average.cpp"), "-o", exe, f"-L{LIB}", "-lkzhip", f"-Wl,-rpath,{LIB}"])
    return exe


def test_library_exports_the_average_entries_and_refuses_a_null_engine():
    lib = capi.load()
    for name in ("kz_engine_eval_packed_decoded_avg", "kz_engine_submit_packed_decoded_avg"):
        assert hasattr(lib, name), name
    assert lib.kz_engine_submit_packed_decoded_avg(None, 0, None, 0, None, 1, None, None) != 0
    assert b"kz_engine_submit_packed_decoded_avg: null engine" in lib.kz_last_error()
    assert lib.kz_engine_eval_packed_decoded_avg(None, None, 0, None, 1, None, None, None, None) != 0
    assert b"kz_engine_eval_packed_decoded_avg: null engine" in lib.kz_last_error()


def test_numpy_average_is_the_stated_arithmetic():
    """average_f32 — the yardstick's reduction — on random probabilities: float32 throughout, within the roundings of n
    quotients and n additions of the float64 average, exact where the arithmetic is (n = 1; equal terms at n = 8), and its
    layout is virtual board b * n + k = board b under symmetry k."""
    from tests.test_gpu_symmetry_average import average_f32, replicated
    rng = np.random.default_rng(7)
    for n_sym in (1, 3, 8):
        batch = 5
        lens = [0, 1, 17, 60, 33]
        values = rng.standard_normal((batch * n_sym, 5)).astype(np.float32)
        probs = [rng.random(lens[v // n_sym]).astype(np.float32) for v in range(batch * n_sym)]
        v, p = average_f32(values, probs, n_sym)
        assert v.shape == (batch, 5) and v.dtype == np.float32 and [len(x) for x in p] == lens
        v64 = values.astype(np.float64).reshape(batch, n_sym, 5).mean(axis=1)
        # n additions and one division (values), n divisions and n additions (probabilities), each within 2^-24 relative of a
        # partial result no larger than sum |terms|
        u = 2.0 ** -24
        assert np.all(np.abs(v - v64) <= (n_sym + 1) * u * np.abs(values).astype(np.float64).reshape(batch, n_sym, 5).sum(axis=1) * 1.01)
        for b in range(batch):
            p64 = np.mean([probs[b * n_sym + k].astype(np.float64) for k in range(n_sym)], axis=0) if lens[b] else np.zeros(0)
            assert p[b].dtype == np.float32 and np.all(np.abs(p[b] - p64) <= 2 * n_sym * u * p64 * 1.01)
        if n_sym == 1:
            assert np.array_equal(v, values) and all(np.array_equal(a, b) for a, b in zip(p, probs))
    # by hand: ((0 + 1/8) + ... ) of eight ones is exactly one; the order is k ascending (a sum that depends on it)
    v, p = average_f32(np.ones((8, 5), np.float32), [np.ones(2, np.float32)] * 8, 8)
    assert np.array_equal(v, np.ones((1, 5), np.float32)) and np.array_equal(p[0], np.ones(2, np.float32))
    big = np.array([2.0 ** 24, 1.0, 1.0], np.float32)  # ((2^24 + 1) + 1) = 2^24 in f32; ((1 + 1) + 2^24) = 2^24 + 2
    v, _ = average_f32(np.repeat(big[:, None], 5, axis=1), [np.zeros(0, np.float32)] * 3, 3)
    assert np.array_equal(v[0], np.full(5, np.float32(2.0 ** 24) / np.float32(3), np.float32))
    v, _ = average_f32(np.repeat(big[::-1][:, None], 5, axis=1), [np.zeros(0, np.float32)] * 3, 3)
    assert np.array_equal(v[0], np.full(5, np.float32(2.0 ** 24 + 2) / np.float32(3), np.float32))
    # the replicated batch: board-major, ids 0 .. n-1 within a board
    bits = np.arange(6, dtype=np.uint8).reshape(3, 2)
    r_bits, r_scalars, r_moves, ids = replicated(bits, np.arange(3, dtype=np.float32)[:, None], [[1], [2, 3], []], 2)
    assert r_bits[:, 0].tolist() == [0, 0, 2, 2, 4, 4] and r_scalars[:, 0].tolist() == [0, 0, 1, 1, 2, 2]
    assert r_moves == [[1], [1], [2, 3], [2, 3], [], []] and ids.tolist() == [0, 1, 0, 1, 0, 1] and ids.dtype == np.uint8


def test_hip_symmetry_average_test_compiles_against_the_c_abi():
    _build_hip_test()


@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_device_average_equals_the_host_wrapper_on_gpu():
    """HipNetwork::set_average_symmetries against AverageSymmetryNetwork<AtaxxSymBoard, HipNetwork> on the golden Ataxx network:
    equal values, per-move probabilities within the bound the C++ file derives."""
    exe = _build_hip_test()
    out = subprocess.run([exe, os.path.join(GOLDEN, "ataxx7_2x16.kzm")], capture_output=True, text=True, timeout=200)
    assert out.returncode == 0 and "hip symmetry average tests ok" in out.stdout, out.stdout + out.stderr
