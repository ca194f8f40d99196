"""Networks for the per-layer f16 and split16 board-tile kernels ("board_conv_f16", "board_conv_split16": kz_board_conv.hip), on
the draws, boards and float64 reference of tests/exact_nets.py (`draw_exact`, `exact_boards`, `reference`, the wide family, SEED,
BOARDS) and the geometry rule of tests/int8_board_nets.py (`geometry`): only the table of networks is new.  Test infrastructure
only, no GPU.

Neither kernel is templated by shape: chunk count, output-channel quarters, boards per workgroup, tiles per board, line skew and
the padding-tile skip are runtime values.  The networks are chosen by what those values become, each at depth 1 unless the depth
is the point; `NETS` says which is there for what, tests/test_board_nets.py pins the values, tests/test_gpu_board_exact.py runs
the engines.  Three faults of such a kernel that no network of depth 1 and at most 128 channels can show are mutants of the
reference (`exact_nets.reference`, spoil=): a stale middle chunk, a residual from the wrong quarter, a residual from a buffer
that was never rotated (`mutants`)."""
import numpy as np

from kzero_amd.model_file import write_model
from tests import exact_nets as E
from tests import int8_board_nets as I

NORES = {"KZ_NO_RESIDENT_F16G": "1"}  # the f16 selector's one-launch tower would take the shape
_Q64 = dict(query_channels=64)

# name -> (game, depth, channels, head, synth.random_model keywords, {dense position: density < 1}, max_batch, switches of the
#          f16 engine, whether the split16 selector sends the shape to the board kernel)
# max_batch: the f16 selector wants >= 160 workgroups at max_batch (groups x quarters); every engine of a network takes the same.
# Comments: tiles per board / boards per workgroup / skew (test_geometry_is_what_the_table_says), chunks of 64 (f16) and of 32
# (split16), output-channel quarters nq.
NETS = {
    # the shipping width: 23 tiles, one board, skewed lines, the padding tile skipped; f16 four chunks, two of them neither first
    # nor last; split16 eight; nq = 4.  Conv B dense holds the sums at half density only (a 2304-term row of a 19x19 board).
    "go19_1x256": ("go-19", 1, 256, "conv", {}, {2: 0.5}, 256, {}, True),
    # three chunks (odd; split16 six), nq = 3: not a power of two
    "go19_1x192": ("go-19", 1, 192, "conv", {}, {}, 256, {}, True),
    # depth 2: the rotation of the three activation buffers wraps, block 2's residual lies two buffers back.  11 tiles, two boards
    # in 22 tiles, two idle tiles that are NOT skipped (the skip needs exactly one).  The split instance on 13x13.
    "go13_2x128": ("go-13", 2, 128, "conv", {}, {}, 256, NORES, True),
    # six tiles, four boards in 24 tiles, boards straddle tiles, unskewed lines; the split instance on a small board
    "go9_1x256": ("go-9", 1, 256, "conv", {}, {}, 256, NORES, True),
    # four tiles, six boards, unskewed lines of 8 slots; six chunks (split16 twelve), nq = 6
    "ataxx7_1x384": ("ataxx-7", 1, 384, "ataxx_conv", {}, {}, 256, NORES, True),
    # 8x8: four tiles, five boards in 20 tiles (the LDS holds no sixth), four idle tiles, every board edge a tile edge; five
    # chunks, nq = 5; the attention heads behind the per-layer tower.  320 channels is no shape of the one-launch split tower.
    "chess_1x320_att": ("chess", 1, 320, "attention", _Q64, {}, 256, NORES, True),
    # two tiles a board, 11 boards in 22 tiles: the LDS sets the boards per workgroup, not the 24 tiles
    "ataxx5_1x128": ("ataxx-5", 1, 128, "ataxx_conv", {}, {}, 1024, NORES, False),
    # three tiles a board (the reciprocal of 3), eight boards
    "ataxx6_1x128": ("ataxx-6", 1, 128, "ataxx_conv", {}, {}, 1024, NORES, False),
    # one tile a board, every board edge a tile edge; 16 boards, again by the LDS (24 tiles would hold 24)
    "ataxx4_1x128": ("ataxx-4", 1, 128, "ataxx_conv", {}, {}, 2048, NORES, False),
    # 128 channels on at most 96 squares is a shape of the one-launch split tower, which no switch turns off: the three networks
    # above run the f16 instance only and have no wide variants (the split16 engines' family).  The same three geometries at
    # 320 channels, the nearest width the split selector sends to the board kernel on any board: both instances, nq = 5
    "ataxx5_1x320": ("ataxx-5", 1, 320, "ataxx_conv", {}, {}, 512, NORES, True),
    "ataxx6_1x320": ("ataxx-6", 1, 320, "ataxx_conv", {}, {}, 256, NORES, True),
    "ataxx4_1x320": ("ataxx-4", 1, 320, "ataxx_conv", {}, {}, 512, NORES, True),
    # tests/test_gpu_exact.py runs it in f16; here for the split instance on 13x13 at depth 1, wide variants included
    "go13_1x128": ("go-13", 1, 128, "conv", {}, {}, 256, NORES, True),
}
SEED = E.SEED
BOARDS = E.BOARDS
# cases whose first draw misses a condition: (network, dense position, wide variant) -> the seed draw_exact settles on (SEED + 1000 k)
REDRAWN = {("ataxx6_1x320", 2, None): 1001}  # conv B dense at 320 channels: a sum of the first draw passes 2^22 steps

# where each mutant kind applies (module docstring); the first three networks of tests/test_gpu_exact.py's board engines have none
CHUNK_NETS = QUARTER_NETS = ("go19_1x256", "go19_1x192", "go9_1x256", "ataxx7_1x384", "chess_1x320_att", "ataxx5_1x320", "ataxx6_1x320",
                            "ataxx4_1x320")
STALE_NETS = ("go13_2x128",)
BEFORE = ("go19_1x64", "go19_1x128", "go13_1x128")  # exact_nets.NETS: what the board engines ran before this table


def size(net):
    return {"chess": 8}.get(NETS[net][0]) or int(NETS[net][0].split("-")[1])


def geometry(net):
    """(tiles per board, boards per workgroup, skew16): int8_board_nets.geometry, the rule all three board-tile kernels share."""
    return I.geometry(size(net), size(net))


def workgroups(net, boards):
    """Workgroups of a launch: int8_board_nets.workgroups counts 64-channel quarters of a tower widened to a multiple of 128, so
    at 128 channels it is two per board group; these kernels take the width as it is."""
    return I.workgroups(boards, size(net), size(net), 128) // 2 * (NETS[net][2] // 64)


def launches(net):
    """Board counts of the three launches: nine board groups, the last of one board (the ninth group wraps to slot 1 of XCD 0, the
    other seven workgroups of that slot row return early); two groups; one board alone."""
    bpw = geometry(net)[1]
    return [8 * bpw + 1, bpw + 1, 1]


def dense_positions(net):
    """None, the stem, every tower convolution.  The heads are not these kernels'."""
    return [None] + list(range(2 * NETS[net][1] + 1))


def wide_positions(net):
    """(at, side) of every wide variant that touches the tower: the scalar planes, the stem, each tower convolution; attention
    heads twice, q_from or q_to narrow (exact_nets.wide_positions)."""
    if not NETS[net][8]:
        return []
    sides = ("from", "to") if NETS[net][3] == "attention" else (None,)
    return [(at, side) for side in sides for at in ["input"] + list(range(2 * NETS[net][1] + 1))]


_CACHE = {}
_COVER = {}


def build(net, dense_at, wide=None):
    """exact_nets.build on this module's table: one model per (network, dense position, wide variant) with its boards and
    float64 reference; the last few are kept."""
    key = (net, dense_at, wide)
    if key not in _CACHE:
        while len(_CACHE) >= 4:
            _CACHE.pop(next(iter(_CACHE)))
        game, depth, channels, head, kw, density_at = NETS[net][:6]
        b = E.Built()
        b.bits, b.scalars_in = E.exact_boards(game, BOARDS, SEED, wide=wide is not None and wide[0] == "input")
        b.meta, b.tensors, b.seed, (s, p, b.report) = E.draw_exact(game, depth, channels, head, dense_at, SEED, boards=(b.bits, b.scalars_in),
                                                                   density=density_at.get(dense_at, 1.0), wide=wide, **kw)
        b.blob = write_model(b.meta, b.tensors)
        b.x = E.encode(b.meta, b.bits, b.scalars_in)
        b.ref_scalars, b.ref_policy = s.astype(np.float32), p.astype(np.float32)
        b.layers = E.layer_names(b.tensors)
        _CACHE[key] = b
        if wide is not None:
            _COVER[net, wide] = (b.report.lo_in, b.report.lo_w)
    return _CACHE[key]


def coverage(net):
    """{wide variant: (lo_in, lo_w)} over the network's wide variants."""
    for wide in wide_positions(net):
        if (net, wide) not in _COVER:
            build(net, None, wide)
    return {wide: _COVER[net, wide] for wide in wide_positions(net)}


def mutants(net):
    """{name: spoil} of every mutant reference the network can express: the first block's conv A with a stale chunk k for each k
    that is neither first nor last; block 1's residual quarter q from q - 2 for each q >= 2; block 2's residual block 1's input."""
    depth, channels = NETS[net][1], NETS[net][2]
    m = {f"chunk-{k}": dict(layer="common.tower.1.seq.0", chunk=k) for k in range(1, channels // 64 - 1)}
    m.update({f"quarter-{q}": dict(block=1, quarter=q) for q in range(2, channels // 64)})
    if depth >= 2:
        m["stale-residual"] = dict(block=2, stale=True)
    return m
