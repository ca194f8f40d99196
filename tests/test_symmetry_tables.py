"""Board symmetries inside the launch, the parts that need no GPU: the tables the host mirror builds for the engine
(kzero_amd/csrc/host/symmetry.hpp: SymmetryTables, d4_tables) against the reference's own Ataxx tables and the host's board
mapping — a C++ unit, built and run like tests/cpp/test_host.cpp —, the numpy host route of tests/test_gpu_symmetry.py against
those tables, and the new entries in the built library.  The GPU half of the C++ mirror (HipNetwork::set_random_symmetries
against the RandomSymmetryNetwork wrapper) is tests/cpp/test_hip_symmetry.cpp, run here under -m gpu."""
import os
import subprocess

import numpy as np
import pytest

from kzero_amd import capi, synth

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(REPO, "tests", "cpp")
BUILD = os.path.join(CPP, "build")
GOLDEN = os.path.join(REPO, "tests", "golden")
LIB = os.path.join(REPO, "kzero_amd")


def _build(src, out, extra=()):
    os.makedirs(BUILD, exist_ok=True)
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-pthread", os.path.join(CPP, src), "-o",
           os.path.join(BUILD, out), *extra]
    subprocess.check_call(cmd)
    return os.path.join(BUILD, out)


@pytest.fixture(scope="module")
def tables_exe():
    return _build("test_symmetry_tables.cpp", "test_symmetry_tables_asan",
                  ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])


def test_symmetry_tables_cpp_unit(tables_exe):
    """d4_tables(AtaxxStdMapper) == tests/golden/ataxx_symmetry.txt (7 sizes x 8 symmetries), square_src consistent with
    ataxx_map_tiles, the Go tables (9, 19) permutations with the policy map agreeing with the square map and pass fixed,
    tables applied to a packed AtaxxSymBoard == packing board.map(sym)."""
    out = subprocess.run([tables_exe, GOLDEN], capture_output=True, text=True, timeout=200)
    assert out.returncode == 0 and "symmetry table tests ok" in out.stdout, out.stdout + out.stderr


def test_python_go_formula_is_the_host_mirrors_table(tables_exe):
    """The Go tables tests/test_gpu_symmetry.py computes from the D4 formula are the ones d4_tables(GoStdMapper) hands the engine."""
    from tests.test_gpu_symmetry import go_tables
    out = subprocess.run([tables_exe, "dump-go", "9"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    rows = [ln.split("|") for ln in out.stdout.splitlines()]
    square_src, policy_map = go_tables(9)
    assert np.array_equal(np.array([r[0].split() for r in rows], np.int32), square_src)
    assert np.array_equal(np.array([r[1].split() for r in rows], np.int32), policy_map)


def test_numpy_host_route_on_the_reference_tables():
    """The yardstick of the GPU tests, checked where a symmetry is known by hand: under the reference's Ataxx tables a tile
    lands where the copy move to it lands, the mapping of a board by g then its inverse is the board, the move lists keep
    their order."""
    from tests.test_gpu_symmetry import ataxx_tables, map_bits, map_moves
    square_src, policy_map = ataxx_tables(7)
    assert np.array_equal(square_src[0], np.arange(49)) and np.array_equal(policy_map[0][policy_map[0] >= 0],
                                                                            np.flatnonzero(policy_map[0] >= 0))
    bits, _ = synth.random_boards("ataxx-7", 16, seed=3)
    planes = np.unpackbits(bits, axis=1, bitorder="little")[:, :147].reshape(16, 3, 49)
    ids = (np.arange(16) % 8).astype(np.uint8)
    mapped = np.unpackbits(map_bits(bits, 3, 49, square_src, ids), axis=1, bitorder="little")[:, :147].reshape(16, 3, 49)
    for b in range(16):
        for tile in range(49):
            assert np.array_equal(mapped[b, :, policy_map[ids[b], tile]], planes[b, :, tile])
    # index 1 = flip_y alone, index 4 = transpose alone: involutions
    for s in (1, 2, 4):
        twice = map_bits(map_bits(bits, 3, 49, square_src, np.full(16, s)), 3, 49, square_src, np.full(16, s))
        assert np.array_equal(twice[:, :18], bits[:, :18])
    moves = [np.array([5, 833, 60, 0], np.int32)] * 16
    out = map_moves(moves, policy_map, ids)
    assert all(m[1] == 833 for m in out) and [int(m[0]) for m in out] == [int(policy_map[i, 5]) for i in ids]


def test_library_exports_the_symmetry_entries_and_refuses_a_null_engine():
    lib = capi.load()
    for name in ("kz_engine_set_symmetries", "kz_engine_eval_packed_decoded_sym", "kz_engine_submit_packed_decoded_sym"):
        assert hasattr(lib, name), name
    one = np.zeros(1, np.int32)
    assert lib.kz_engine_set_symmetries(None, 1, one.ctypes.data, one.ctypes.data) != 0
    assert b"null argument" in lib.kz_last_error()
    assert lib.kz_engine_submit_packed_decoded_sym(None, 0, None, 0, None, 1, None, None, None) != 0
    assert b"kz_engine_submit_packed_decoded_sym" in lib.kz_last_error()


def test_hip_symmetry_test_compiles_against_the_c_abi():
    _build("test_hip_symmetry.cpp", "test_hip_symmetry", [f"-L{LIB}", "-lkzhip", f"-Wl,-rpath,{LIB}"])


@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_device_symmetries_equal_the_host_wrapper_on_gpu(tmp_path):
    """HipNetwork::set_random_symmetries against RandomSymmetryNetwork<HipNetwork> with the same id sequence, Ataxx 2 x 64:
    equal values, per-move probabilities within 2 n 2^-24 relative (the order of one softmax sum)."""
    exe = _build("test_hip_symmetry.cpp", "test_hip_symmetry", [f"-L{LIB}", "-lkzhip", f"-Wl,-rpath,{LIB}"])
    model = tmp_path / "ataxx7_2x64.kzm"
    model.write_bytes(synth.random_model("ataxx-7", 2, 64, "ataxx_conv", seed=5))
    out = subprocess.run([exe, str(model)], capture_output=True, text=True, timeout=200)
    assert out.returncode == 0 and "hip symmetry tests ok" in out.stdout, out.stdout + out.stderr
