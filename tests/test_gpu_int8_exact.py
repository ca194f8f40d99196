"""KZ_DTYPE_INT8 on the GPU, to the bit (tests/int8_nets.py): the one-launch int8 tower must return the bits of the float64
reference that quantises where the launch quantises.  Integer sums are exact and every scale is a power of two, so there is
no tolerance: a difference is an indexing, packing, lane-map, rounding or clamping error.

Both families on every instance of the table in kz_tower_i8.hip: chess 2x256 (the attention head outside the launch), chess
1x256 (the last-layer epilogue alone), chess-hist-1 1x256 (two stem chunks), chess 2x128 (four tiles at 128 channels), ataxx7 2x128 (two boards in seven tiles) and
go9 3x128 (one board in six), on an engine
of max_batch 64 — 13 boards, one board, boards per workgroup + 1 (the ragged last workgroup) — and, at 256 channels, on an
engine large enough for two boards per workgroup, on an odd board count.  The exact family also with each block convolution in
turn carrying asymmetric weights on every lane of its fragments.  The heads behind the tower are f16 kernels on values they hold
exactly (int8_nets.head_conditions), so the tower alone decides the bits.  On a mismatch the test prints which one-site-less
reference the output equals."""
import numpy as np
import pytest

from kzero_amd import capi
from tests import int8_nets as N
from tests.test_gpu_exact import mismatch

pytestmark = pytest.mark.gpu

INT8 = capi.KZ_DTYPE_INT8
MAX_BATCH = 64
WIDE_BATCH = 256   # ceil(256 / 2) = 128 workgroups of two boards: the two-board instance at 256 channels
WIDE_BOARDS = 255  # an odd count that still selects it: the last workgroup holds one board
PER = {"chess_2x256_att": 1, "chess_1x256_att": 1, "chesshist1_1x256_att": 1, "chess_2x128_att": 1, "ataxx7_2x128": 2, "go9_3x128": 1}  # boards per workgroup at max_batch 64
CASES = [(net, "exact", d) for net in N.NETS for d in N.dense_positions(net)] + [(net, "round", None) for net in N.NETS]
IDS = [f"{net}-{fam}-{d}" for net, fam, d in CASES]


@pytest.fixture(scope="module")
def dev():
    assert capi.device_count() >= 1
    return 0


def which_mutant(b, s, p, idx):
    hits = []
    for name, m in N.mutants(b).items():
        if name.startswith("without-"):
            ms, mp = N.run_mutant(b, m)
            if np.array_equal(s, ms[idx]) and np.array_equal(p, mp[idx]):
                hits.append(name)
    return f"equals the reference {' / '.join(hits)}" if hits else "equals no one-site-less reference"


def check(b, eng, idx, what):
    hw = b.meta["board_h"] * b.meta["board_w"]
    s, p = eng.eval_packed(b.bits[idx], b.scalars_in[idx])
    if not (np.array_equal(s, b.ref_scalars[idx]) and np.array_equal(p, b.ref_policy[idx])):
        print(f"[int8] {what}: {which_mutant(b, s, p, idx)}")
    assert np.array_equal(s, b.ref_scalars[idx]), f"{what}, scalars: " + mismatch(s, b.ref_scalars[idx], 5)
    assert np.array_equal(p, b.ref_policy[idx]), f"{what}, policy: " + mismatch(p, b.ref_policy[idx], hw)


@pytest.mark.parametrize("net,family,dense_at", CASES, ids=IDS)
def test_int8_engine_returns_the_reference_bits(dev, net, family, dense_at):
    b = N.build_exact(net, dense_at) if family == "exact" else N.build_round(net, dense_at)
    depth = b.meta["tower_depth"]
    assert all(b.report.exact.values()) and N.head_conditions(b.heads, depth)
    model = capi.Model(blob=b.blob).quantize_int8(b.site_max)
    assert list(model.int8_site_exponents()) == b.exps[:2 * depth]
    eng = capi.Engine(model, dev, MAX_BATCH, INT8)
    assert eng.tower_path == "tower_resident_i8"
    per = PER[net]
    assert eng.launch_geometry(N.BOARDS) == ((N.BOARDS + per - 1) // per, per)
    for n in (N.BOARDS, 1, per + 1):
        check(b, eng, np.arange(n), f"{net} {family} {dense_at}, {n} boards")
    if b.meta["tower_channels"] == 256 and dense_at is None:
        wide = capi.Engine(model, dev, WIDE_BATCH, INT8)
        assert wide.tower_path == "tower_resident_i8"
        assert wide.launch_geometry(WIDE_BOARDS) == ((WIDE_BOARDS + 1) // 2, 2)
        assert wide.launch_geometry(N.BOARDS) == (N.BOARDS, 1)  # (too few boards to fill 128 such workgroups: one per workgroup)
        check(b, wide, np.arange(WIDE_BOARDS) % N.BOARDS, f"{net} {family}, two boards per workgroup, {WIDE_BOARDS} boards")
