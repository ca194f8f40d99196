"""KZ_DTYPE_INT8_HEADS on the GPU, to the bit: "tower_resident_i8+heads" must return the bits of tests/int8_nets.py's
references, unchanged — the tower is dtype 4's, and the heads inside the launch are f16 MFMAs and f32 sums on values they hold
exactly (int8_nets.head_conditions), in any order of summation.  No tolerance: a difference is an indexing, packing, lane-map or
staging error of the head pass, the small convolutions or the tail.

Every network of int8_nets.NETS whose heads the launch carries — two, one, four and three boards per workgroup in seven, six
and four tiles at 128 channels (one widened from 96), four, two and one at 256 — in the exact family at each of its
dense_positions and in the rounding family, and the two conv-head networks of WEIGHT_NETS with weights that round.  Each on an
engine of max_batch 64: 13 boards, one board, boards per workgroup + 1 and twice that + 1 through the packed entry, the 13
through kz_engine_eval_dense too; the same bits as a dtype-4 engine of the same model.  One 256-channel network on an engine
of max_batch 256 with 255 boards: where dtype 4 takes two boards per workgroup, the launch with the heads inside keeps one."""
import numpy as np
import pytest

from kzero_amd import capi, synth
from tests import int8_nets as N
from tests.test_gpu_int8_exact import same_bits

pytestmark = pytest.mark.gpu

HEADS, INT8 = capi.KZ_DTYPE_INT8_HEADS, capi.KZ_DTYPE_INT8
PATH = "tower_resident_i8+heads"
MAX_BATCH = 64
WIDE_BATCH, WIDE_BOARDS = 256, 255
# the networks of N.NETS the launch carries the heads of (tests/test_int8_heads_api.py holds the rule): boards per workgroup
FUSED = {"ataxx7_2x128": 2, "go9_3x128": 1, "ataxx5_2x128": 4, "ataxx6_2x128": 3, "ataxx7_2x96": 2, "ataxx4_2x256": 4,
         "ataxx5_2x256": 2, "ataxx6_2x256": 1, "ataxx7_2x256": 1}
CASES = ([(net, "exact", d) for net in FUSED for d in N.dense_positions(net)] + [(net, "round", None) for net in FUSED] +
         [(net, "weights", None) for net in N.WEIGHT_NETS if net in FUSED])
IDS = [f"{net}-{fam}-{d}" for net, fam, d in CASES]
assert all(N.NETS[net][1] <= 3 for net in FUSED) and len([c for c in CASES if c[1] == "weights"]) == 2


@pytest.fixture(scope="module")
def dev():
    assert capi.device_count() >= 1
    return 0


@pytest.mark.parametrize("net,family,dense_at", CASES, ids=IDS)
def test_heads_inside_the_launch_return_the_reference_bits(dev, net, family, dense_at):
    b = N.build_exact(net, dense_at) if family == "exact" else N.build_round(net, dense_at, "round" if family == "weights" else None)
    depth, channels, hw = b.meta["tower_depth"], b.meta["tower_channels"], b.meta["board_h"] * b.meta["board_w"]
    assert all(b.report.exact.values()) and N.head_conditions(b.heads, depth)
    model = capi.Model(blob=b.blob).quantize_int8(b.site_max)
    eng = capi.Engine(model, dev, MAX_BATCH, HEADS)
    assert eng.tower_path == PATH
    per = N.boards_per_workgroup(channels, hw)
    assert per == FUSED[net] <= 4
    assert eng.launch_geometry(N.BOARDS) == ((N.BOARDS + per - 1) // per, per)
    four = capi.Engine(model, dev, MAX_BATCH, INT8)
    assert four.tower_path == "tower_resident_i8"
    for n in dict.fromkeys((N.BOARDS, 1, per + 1, 2 * per + 1)):
        idx = np.arange(n) % N.BOARDS
        what = f"{net} {family} {dense_at}, {n} boards"
        s, p = eng.eval_packed(b.bits[idx], b.scalars_in[idx])
        same_bits(b, s, p, idx, what)
        s4, p4 = four.eval_packed(b.bits[idx], b.scalars_in[idx])
        assert np.array_equal(s, s4) and np.array_equal(p, p4), what + ": differs from the dtype-4 engine"
        if n == N.BOARDS:  # the unpacked entry: the encode the reference itself consumed
            s, p = eng.eval_dense(b.x[idx])
            same_bits(b, s, p, idx, what + ", eval_dense")


def test_one_board_per_workgroup_at_256_channels_whatever_the_batch(dev):
    net = "ataxx7_2x256"
    b = N.build_exact(net, None)
    model = capi.Model(blob=b.blob).quantize_int8(b.site_max)
    eng = capi.Engine(model, dev, WIDE_BATCH, HEADS)
    assert eng.tower_path == PATH
    assert eng.launch_geometry(WIDE_BOARDS) == (WIDE_BOARDS, 1)
    idx = np.arange(WIDE_BOARDS) % N.BOARDS
    s, p = eng.eval_packed(b.bits[idx], b.scalars_in[idx])
    same_bits(b, s, p, idx, f"{net}, {WIDE_BOARDS} boards on an engine of {WIDE_BATCH}")
    # ... and on the one board where dtype 4 does take two per workgroup at that batch, 8x8 (no network of int8_nets has a conv
    # head on it: a random one, held to the bits the same arithmetic returns on an engine too small for the wide tiles)
    blob = synth.random_model("ataxx-8", 2, 256, "ataxx_conv", seed=5)
    bits, scalars = synth.random_boards("ataxx-8", WIDE_BOARDS, seed=3)
    model = capi.calibrate_int8(capi.Model(blob=blob), dev, bits[:32], scalars[:32], headroom=2.0)
    wide4, wide5, small5 = (capi.Engine(model, dev, mb, dt) for mb, dt in ((WIDE_BATCH, INT8), (WIDE_BATCH, HEADS), (MAX_BATCH, HEADS)))
    assert wide4.launch_geometry(WIDE_BOARDS) == ((WIDE_BOARDS + 1) // 2, 2)
    assert wide5.tower_path == small5.tower_path == PATH and wide5.launch_geometry(WIDE_BOARDS) == (WIDE_BOARDS, 1)
    s, p = wide5.eval_packed(bits, scalars)
    assert np.isfinite(s).all() and np.isfinite(p).all()
    for lo in range(0, WIDE_BOARDS, MAX_BATCH):
        s_small, p_small = small5.eval_packed(bits[lo:lo + MAX_BATCH], scalars[lo:lo + MAX_BATCH])
        assert np.array_equal(s_small, s[lo:lo + MAX_BATCH]) and np.array_equal(p_small, p[lo:lo + MAX_BATCH]), lo
