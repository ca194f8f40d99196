"""KZ_DTYPE_INT8 on the GPU, to the bit (tests/int8_nets.py): the one-launch int8 tower must return the bits of the float64
reference that quantises where the launch quantises.  Integer sums are exact and every scale is a power of two, so there is
no tolerance: a difference is an indexing, packing, lane-map, rounding or clamping error.

Both families on every instance of the table in kz_tower_i8.hip: chess 2x256 (the attention head outside the launch), chess
1x256 (the last-layer epilogue alone), chess-hist-1 1x256 (two stem chunks), chess 2x128 (four tiles at 128 channels), ataxx7
2x128 (two boards in seven tiles) and go9 3x128 (one board in six), the exact family of these six also with each block
convolution in turn carrying asymmetric weights on every lane of its fragments.  Then the square-board geometries the plan
accepts beside those (the table of int8_nets.NETS says which network is there for what): 3, 4, 7, 12 and 28 boards per
workgroup at 128 channels, 2, 4, 7 (3x3: one idle row) and 16 at 256, one board with 15 and with 28 idle rows, three and four
stem chunks, towers widened from 96 and 200 channels, three block boundaries — these with no dense layer, the first conv A
dense and the last conv B dense.  And the rounding family with weights that round
(int8_nets.WEIGHT_NETS, one network per instance): ties in both directions, every bit of a weight byte.

Every case on an engine of max_batch 64: 13 boards, one board, boards per workgroup + 1 (the ragged last workgroup) and twice
the boards per workgroup + 1 (two full workgroups and a ragged one: with more than 13 boards per workgroup nothing else fills
one), through the packed entry, and the 13 boards through kz_engine_eval_dense as well (the encoded planes the reference itself
consumed: the launch's unpacked input path).  The chess networks at 256 channels (widened from 200 among them) also on an
engine large enough for two boards per workgroup, on an odd board count.  The heads behind the tower are f16 kernels on values
they hold exactly (int8_nets.head_conditions), so the tower alone decides the bits.  On a mismatch the test prints which
one-site-less reference, or which reference that rounds the weights otherwise, the output equals."""
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
CASES = ([(net, "exact", d) for net in N.NETS for d in N.dense_positions(net)] + [(net, "round", None) for net in N.ROUND_NETS] +
         [(net, "weights", None) for net in N.WEIGHT_NETS])
IDS = [f"{net}-{fam}-{d}" for net, fam, d in CASES]


@pytest.fixture(scope="module")
def dev():
    assert capi.device_count() >= 1
    return 0


def which_mutant(b, s, p, idx):
    hits = []
    for name, m in N.mutants(b).items():
        if name.startswith(("without-", "weights-")):
            ms, mp = N.run_mutant(b, m)
            if np.array_equal(s, ms[idx]) and np.array_equal(p, mp[idx]):
                hits.append(name)
    return f"equals the reference {' / '.join(hits)}" if hits else "equals no one-site-less or weight-rounding reference"


def same_bits(b, s, p, idx, what):
    hw = b.meta["board_h"] * b.meta["board_w"]
    if not (np.array_equal(s, b.ref_scalars[idx]) and np.array_equal(p, b.ref_policy[idx])):
        print(f"[int8] {what}: {which_mutant(b, s, p, idx)}")
    assert np.array_equal(s, b.ref_scalars[idx]), f"{what}, scalars: " + mismatch(s, b.ref_scalars[idx], 5)
    assert np.array_equal(p, b.ref_policy[idx]), f"{what}, policy: " + mismatch(p, b.ref_policy[idx], hw)


def check(b, eng, idx, what, dense=False):
    s, p = eng.eval_packed(b.bits[idx], b.scalars_in[idx])
    same_bits(b, s, p, idx, what)
    if dense:  # the unpacked entry: the encode the reference itself consumed
        s, p = eng.eval_dense(b.x[idx])
        same_bits(b, s, p, idx, what + ", eval_dense")


@pytest.mark.parametrize("net,family,dense_at", CASES, ids=IDS)
def test_int8_engine_returns_the_reference_bits(dev, net, family, dense_at):
    b = N.build_exact(net, dense_at) if family == "exact" else N.build_round(net, dense_at, "round" if family == "weights" else None)
    depth, channels, hw = b.meta["tower_depth"], b.meta["tower_channels"], b.meta["board_h"] * b.meta["board_w"]
    assert all(b.report.exact.values()) and N.head_conditions(b.heads, depth)
    model = capi.Model(blob=b.blob).quantize_int8(b.site_max)
    assert list(model.int8_site_exponents()) == b.exps[:2 * depth]
    eng = capi.Engine(model, dev, MAX_BATCH, INT8)
    assert eng.tower_path == "tower_resident_i8"
    per = N.boards_per_workgroup(channels, hw)  # (the rule, from the channels and the board: tests/test_int8_nets.py pins it)
    assert eng.launch_geometry(N.BOARDS) == ((N.BOARDS + per - 1) // per, per)
    assert 2 * per + 1 <= MAX_BATCH
    for n in dict.fromkeys((N.BOARDS, 1, per + 1, 2 * per + 1)):
        check(b, eng, np.arange(n) % N.BOARDS, f"{net} {family} {dense_at}, {n} boards", dense=n == N.BOARDS)
    if N.widened(channels) == 256 and hw == 64 and dense_at is None:
        wide = capi.Engine(model, dev, WIDE_BATCH, INT8)
        assert wide.tower_path == "tower_resident_i8"
        assert wide.launch_geometry(WIDE_BOARDS) == ((WIDE_BOARDS + 1) // 2, 2)
        assert wide.launch_geometry(N.BOARDS) == (N.BOARDS, 1)  # (too few boards to fill 128 such workgroups: one per workgroup)
        check(b, wide, np.arange(WIDE_BOARDS) % N.BOARDS, f"{net} {family}, two boards per workgroup, {WIDE_BOARDS} boards")
