"""Networks for the per-layer int8 kernel (KZ_DTYPE_INT8_ANY where the one-launch int8 tower refuses the shape: "board_conv_i8",
kz_board_conv_i8.hip), on the draws of tests/exact_nets.py and the float64 reference of tests/int8_nets.py (`int8_reference`,
`calibration`, `quantise_weights`, `mutants`): the contract is stated per convolution, so the reference is the same and only
the table of networks is new.  Test infrastructure only, no GPU.

The networks are chosen by what the board-tile geometry does with their shape, each at the smallest size that still
exercises it; `NETS` says which is there for what.  `geometry` restates the kernel's rule (24 tiles of 16 squares, a halo image
in two planes of at most 40 KB less the row tables, the 11-slot skew unless it costs a board) so that the tests can pin boards
per workgroup and workgroups without a GPU.

Families, as in int8_nets: exact (nothing rounds, nothing clamps; also with the first conv A / the last conv B dense on the
first three networks), rounding (ties in both directions, non-ties, clamps at both ends; every mutant reference differs), and
the rounding family with weights that round, one network per chunk count (`WEIGHT_NETS`)."""
import numpy as np

from tests import exact_nets as E
from tests import int8_nets as N

NETS = {
    "go19_2x128_conv": ("go-19", 2, 128, "conv", {}),      # 23 tiles, one board per workgroup, tiles across line ends on skewed lines, one chunk, two groups
    "go19_2x256_conv": ("go-19", 2, 256, "conv", {}),      # two chunks: the chunk boundary, four output-channel groups
    "go19_3x192_conv": ("go-19", 3, 192, "conv", {}),      # widened to 256, two block boundaries
    "go13_2x128_conv": ("go-13", 2, 128, "conv", {}),      # 11 tiles, two boards per workgroup, two idle tiles
    "go9_2x256_conv": ("go-9", 2, 256, "conv", {}),        # six tiles, boards straddling tiles: the shape dtype 4 refuses by squares
    "ataxx7_2x384": ("ataxx-7", 2, 384, "ataxx_conv", {}),  # unskewed lines, six boards per workgroup, three chunks (widened to 512: four), six groups
    "ataxx7_2x64": ("ataxx-7", 2, 64, "ataxx_conv", {}),   # a tower at or under one chunk
    "chess_2x192_att": ("chess", 2, 192, "attention", dict(query_channels=64)),  # 8x8, attention heads behind the per-layer tower
}
# one network the one-launch tower takes too (int8_nets.NETS): dtype 8 must return dtype 5's bits there
BOTH_PLANS = "ataxx7_2x128"
DENSE_NETS = ("go19_2x128_conv", "go19_2x256_conv", "go19_3x192_conv")
WEIGHT_NETS = ["go19_2x128_conv", "go19_2x256_conv", "ataxx7_2x384"]  # one, two and four chunks of the widened tower
SEED = E.SEED
# rounding family: network and boards drawn from this seed where the common one loses a mutant ("clamp-128" or "from-f16": no
# such value at the stem's site reaches a channel the heads read) — the first of 2, 3, ... that loses none and keeps the floors
ROUND_SEED = {"go19_2x128_conv": 3, "go19_3x192_conv": 6, "go13_2x128_conv": 3}
BOARDS = E.BOARDS

MT, LDS_MAX, ROWS = 24, 80 * 1024, 384
RM_BYTES = ROWS * 2 + ROWS * 4


def widened(channels):
    """The width of the int8 images: the next multiple of 128."""
    return (channels + 127) // 128 * 128


def _bpw(h, w, skew):
    tpb, line16 = (h * w + 15) // 16, 5 * (w + 1) + skew
    board_bytes = ((h + 2) * line16 + 5) * 16
    by_tiles = MT // tpb if tpb <= MT else 0
    return min(by_tiles, ((LDS_MAX - RM_BYTES) // 2) // board_bytes)


def geometry(h, w):
    """(tiles per board, boards per workgroup, skew16) of the board-tile kernels (kz_board_conv.hip: Geometry)."""
    skew = 11 if _bpw(h, w, 11) == _bpw(h, w, 0) else 0
    return (h * w + 15) // 16, _bpw(h, w, skew), skew


def workgroups(boards, h, w, channels):
    """kz::board_conv_workgroups on the widened tower: 64 output channels per workgroup."""
    bpw = geometry(h, w)[1]
    return ((boards + bpw - 1) // bpw) * (widened(channels) // 64) if bpw else 0


def dense_positions(net):
    depth = NETS[net][1]
    return [None] + ([1, 2 * depth] if net in DENSE_NETS else [])


_CACHE = {}


def _keep(key, make):
    if key not in _CACHE:
        while len(_CACHE) >= 6:
            _CACHE.pop(next(iter(_CACHE)))
        _CACHE[key] = make()
    return _CACHE[key]


def build_exact(net, dense_at=None):
    """int8_nets.build_exact on this module's table."""
    def make():
        game, depth, channels, head, kw = NETS[net]
        bits, scalars = E.exact_boards(game, BOARDS, SEED)
        meta, t, seed, (s, p, rep) = E.draw_exact(game, depth, channels, head, dense_at, SEED, boards=(bits, scalars),
                                                  density=N.EXACT_ENTRIES / (9.0 * channels), **kw)
        step = min(E.step_of(v) for k, v in rep.acts.items() if k.startswith("tower.") and v.ndim == 4)
        b = N._finish(N.Built(), t, meta, bits, scalars, [N.QMAX * min(step, 1.0)] * (2 * depth + 1))
        b.dense_at, b.step = dense_at, step
        b.plain_scalars, b.plain_policy, b.plain_report = s.astype(np.float32), p.astype(np.float32), rep
        return b
    return _keep(("exact", net, dense_at), make)


def build_round(net, dense_at=None, weights=None):
    """int8_nets.build_round on this module's table."""
    def make():
        game, depth, channels, head, kw = NETS[net]
        seed = ROUND_SEED.get(net, SEED)
        bits, scalars = E.exact_boards(game, BOARDS, seed)
        meta, t = E._draw(game, depth, channels, head, dense_at, seed, 1.0, kw)
        N._classes(t, meta)
        if weights == "round":
            N._round_weights(t, meta, seed)
        else:
            assert weights is None
        x = E.encode(meta, bits, scalars)
        b = N._finish(N.Built(), t, meta, bits, scalars, N.calibration(t, meta, x))
        b.dense_at, b.weights = dense_at, weights
        return b
    return _keep(("round", net, dense_at, weights), make)
