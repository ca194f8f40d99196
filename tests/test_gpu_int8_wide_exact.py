"""The int8 launch's wide tiles at 128 channels on the GPU, to the bit: more boards per workgroup change which workgroup and
which tile a board's rows sit in and nothing else — the block convolutions are exact i32 sums, the heads the f16 tail on the same
values in the same k order — so tests/int8_nets.py's references hold every level to zero tolerance, unchanged.

Every case asserts the launch geometry it means to run (a test that silently ran the narrow tiles would show nothing) and derives
its batches from the measured thresholds (kz_tower_i8.hip: the tower alone 256 workgroups; with the heads inside 128, and 342
for sixteen tiles): the batch that fills the level exactly, the largest counts whose last workgroup holds fewer boards, the
largest count that drops a level, the largest that drops to the narrow tiles.  Boards are the reference's 13, indexed
arange(n) % 13, so every workgroup holds other boards at other rows than the one in front of it.  Dtype 5 equals dtype 4 bit
for bit at every batch, whichever level either takes there.

  go9_3x128        dtype 5: three 9x9 boards in sixteen tiles (row 81 in the middle of tile 5), two in eleven, one in six;
                   dtype 4: two in eleven, one in six (sixteen tiles exist with the heads inside only: the tower alone was
                   measured slower in them than in eleven).  Exact and rounding families, weights that round
  ataxx7_2x128     four 7x7 boards in thirteen tiles, two in seven: dtypes 4 and 5, both families and the weights that round
  chess_2x128_att  two 8x8 boards in eight tiles, one in four: dtype 4 (an attention head: outside the launch)
  ataxx5_2x128     eight 5x5 boards in thirteen tiles: dtype 4 (dtype 5 keeps the narrow tiles' four, with its heads inside)
  ataxx-8 2x128    a conv head on 8x8 (random weights: no network of int8_nets has one): with the heads inside four boards do not
                   fit sixteen tiles' tail, so dtype 5 takes two in eight tiles at any batch — the bits of a dtype-5 engine of
                   max_batch 64 evaluated in slices"""
import numpy as np
import pytest

from kzero_amd import capi, synth
from tests import int8_nets as N
from tests.test_gpu_int8_exact import same_bits

pytestmark = pytest.mark.gpu

INT8, HEADS = capi.KZ_DTYPE_INT8, capi.KZ_DTYPE_INT8_HEADS
T_PLAIN, T_HEADS, T_HEADS_16 = 256, 128, 342  # workgroups a level must fill (kz_tower_i8.hip)


def fill(per, workgroups):
    """The smallest batch that gives `workgroups` workgroups of `per` boards."""
    return (workgroups - 1) * per + 1


# net: (engine max_batch, {dtype: [(batch, boards per workgroup)]}) — from the thresholds
GO = (3 * T_HEADS_16, {
    HEADS: [(3 * T_HEADS_16, 3), (3 * T_HEADS_16 - 1, 3), (fill(3, T_HEADS_16), 3),  # 342 workgroups: the last holds three, two, one board
            (fill(3, T_HEADS_16) - 1, 2),                                            # 1023: odd, the largest count of eleven tiles
            (fill(2, T_HEADS), 2), (fill(2, T_HEADS) - 1, 1)],                       # 255: 128 workgroups of two; 254: the narrow tiles
    INT8: [(3 * T_HEADS_16, 2), (fill(2, T_PLAIN), 2), (fill(2, T_PLAIN) - 1, 1)]})  # 513 workgroups of two; 511: 256; 510: narrow
ATAXX7 = (4 * T_PLAIN, {
    HEADS: [(4 * T_PLAIN, 4), (4 * T_HEADS - 1, 4), (4 * T_HEADS - 2, 4), (fill(4, T_HEADS), 4), (fill(4, T_HEADS) - 1, 2)],
    INT8: [(4 * T_PLAIN, 4), (4 * T_PLAIN - 1, 4), (4 * T_PLAIN - 2, 4), (fill(4, T_PLAIN), 4), (fill(4, T_PLAIN) - 1, 2)]})
CHESS = (2 * T_PLAIN + 64, {INT8: [(2 * T_PLAIN + 64, 2), (fill(2, T_PLAIN), 2), (fill(2, T_PLAIN) - 1, 1)]})
ATAXX5 = (8 * T_PLAIN, {INT8: [(8 * T_PLAIN, 8), (fill(8, T_PLAIN) + 2, 8), (fill(8, T_PLAIN), 8), (fill(8, T_PLAIN) - 1, 4)]})
assert GO[1][HEADS][3][0] == 1023 and GO[1][HEADS][5][0] == 254 and ATAXX7[1][HEADS][-1][0] == 508 and ATAXX5[1][INT8][-1][0] == 2040

CASES = [
    ("go9_3x128", "exact", GO), ("go9_3x128", "round", GO), ("go9_3x128", "weights", GO),
    ("ataxx7_2x128", "exact", ATAXX7), ("ataxx7_2x128", "round", ATAXX7), ("ataxx7_2x128", "weights", ATAXX7),
    ("chess_2x128_att", "exact", CHESS), ("chess_2x128_att", "round", CHESS),
    ("ataxx5_2x128", "exact", ATAXX5), ("ataxx5_2x128", "round", ATAXX5),
]
assert all(net in N.NETS and N.NETS[net][1] <= 3 for net, _, _ in CASES) and "go9_3x128" in N.WEIGHT_NETS


@pytest.fixture(scope="module")
def dev():
    assert capi.device_count() >= 1
    return 0


@pytest.mark.parametrize("net,family,plan", CASES, ids=[f"{c[0]}-{c[1]}" for c in CASES])
def test_wide_tiles_return_the_reference_bits(dev, net, family, plan):
    b = N.build_exact(net, None) if family == "exact" else N.build_round(net, None, "round" if family == "weights" else None)
    assert all(b.report.exact.values()) and N.head_conditions(b.heads, b.meta["tower_depth"])
    model = capi.Model(blob=b.blob).quantize_int8(b.site_max)
    max_batch, batches = plan
    engines = {dtype: capi.Engine(model, dev, max_batch, dtype) for dtype in batches}
    assert engines[INT8].tower_path == "tower_resident_i8"
    if HEADS in engines:
        assert engines[HEADS].tower_path == "tower_resident_i8+heads"
    narrow = N.boards_per_workgroup(b.meta["tower_channels"], b.meta["board_h"] * b.meta["board_w"])
    got = {}
    for dtype, eng in engines.items():
        pers = sorted({per for _, per in batches[dtype]})
        assert len(pers) >= 2 and pers[0] == narrow
        for n, per in batches[dtype]:
            idx = np.arange(n) % N.BOARDS
            assert eng.launch_geometry(n) == ((n + per - 1) // per, per), (net, dtype, n)
            assert model.launch_geometry(max_batch, dtype, n) == eng.launch_geometry(n)
            s, p = eng.eval_packed(b.bits[idx], b.scalars_in[idx])
            same_bits(b, s, p, idx, f"{net} {family}, dtype {dtype}, {n} boards, {per} per workgroup")
            got[dtype, n] = (s, p)
    if HEADS in engines:  # dtype 5 equals dtype 4 bit for bit at each batch of either list, whichever level each takes there
        for n in sorted({n for _, n in got}):
            idx = np.arange(n) % N.BOARDS
            pair = [got.get((dtype, n)) or engines[dtype].eval_packed(b.bits[idx], b.scalars_in[idx]) for dtype in (INT8, HEADS)]
            assert np.array_equal(pair[0][0], pair[1][0]) and np.array_equal(pair[0][1], pair[1][1]), (net, n)


def test_a_conv_head_on_8x8_takes_two_boards_with_the_heads_inside(dev):
    boards, small, big = 2 * T_HEADS + 43, 64, 2 * T_PLAIN + 64  # 150 workgroups of two, the last holds one
    blob = synth.random_model("ataxx-8", 2, 128, "ataxx_conv", seed=5)
    bits, scalars = synth.random_boards("ataxx-8", big, seed=3)
    model = capi.calibrate_int8(capi.Model(blob=blob), dev, bits[:32], scalars[:32], headroom=2.0)
    wide5, small5, wide4 = (capi.Engine(model, dev, mb, dt) for mb, dt in ((4 * T_HEADS_16, HEADS), (small, HEADS), (big, INT8)))
    assert wide5.tower_path == small5.tower_path == "tower_resident_i8+heads"
    assert wide5.launch_geometry(4 * T_HEADS_16) == (2 * T_HEADS_16, 2)  # (four boards would fill sixteen tiles: the tail caps it)
    assert wide5.launch_geometry(boards) == ((boards + 1) // 2, 2) and small5.launch_geometry(small) == (small, 1)
    assert wide4.launch_geometry(boards) == (boards, 1) and wide4.launch_geometry(big) == (big // 2, 2)
    s, p = wide5.eval_packed(bits[:boards], scalars[:boards])
    assert np.isfinite(s).all() and np.isfinite(p).all()
    for lo in range(0, boards, small):
        hi = min(lo + small, boards)  # (the last slice is ragged: 43 boards)
        s_small, p_small = small5.eval_packed(bits[lo:hi], scalars[lo:hi])
        assert np.array_equal(s_small, s[lo:hi]) and np.array_equal(p_small, p[lo:hi]), lo
    # ... and the tower alone at two boards in eight tiles: dtype 4's bits do not depend on the level either
    s4, p4 = wide4.eval_packed(bits, scalars)
    small4 = capi.Engine(model, dev, small, INT8)
    for lo in (0, big - small):
        s_small, p_small = small4.eval_packed(bits[lo:lo + small], scalars[lo:lo + small])
        assert np.array_equal(s_small, s4[lo:lo + small]) and np.array_equal(p_small, p4[lo:lo + small]), lo
