"""kz_model_int8_taps on the GPU, to the bit: every stored int8 image and the f16 stream value beside it must be what the float64
reference of tests/int8_nets.py stored at that site — `report.sites[name]` as integers, `report.sites[name + ".x"]`, and at the
last site the reference's tower output.  Integer sums are exact and every scale is a power of two, so there is no tolerance; a
difference is an indexing error of the tap stores (tile, row, channel, site), a wrong instance, or a tap that is not what the
launch stored.  No element is -128 (the fill: nothing no lane wrote) and no stream value NaN where a stream exists; a mid site's
stream is NaN and the last site's image 0 by definition.

  one launch, max_batch 64   the smallest shapes that reach each plain instance of kz_tower_i8.hip's table (CASES says which)
  wide levels                batches derived from the thresholds as tests/test_gpu_int8_wide_exact.py derives them, boards
                             arange(n) % 13: the batch that fills the level and one whose last workgroup is part-filled; each
                             case asserts the geometry it means to run
  dtype 5                    returns dtype 4's taps bit for bit
  per layer, dtype 8         the networks of tests/int8_board_nets.py; and on BOTH_PLANS dtype 8's taps are dtype 5's"""
import numpy as np
import pytest

from kzero_amd import capi
from tests import int8_board_nets as B
from tests import int8_nets as N

pytestmark = pytest.mark.gpu

INT8, HEADS, ANY = capi.KZ_DTYPE_INT8, capi.KZ_DTYPE_INT8_HEADS, capi.KZ_DTYPE_INT8_ANY
MAX_BATCH = 64
T_128, T_256 = 256, 128  # workgroups a wide level of the tower alone must fill, at 128 and at 256 channels (kz_tower_i8.hip)

# network: (family, what it reaches) — at least one case with weights that round (the family with clamps at both ends)
CASES = [
    ("chess_2x128_att", "exact"), ("chess_2x128_att", "weights"),  # 4 tiles
    ("go9_3x128", "round"),                                        # 6 tiles, two block boundaries
    ("ataxx7_2x128", "exact"), ("ataxx7_2x128", "weights"),        # 7 tiles, two boards, rows straddling tiles
    ("chess_2x256_att", "exact"), ("chess_2x256_att", "round"),    # 256 channels, 4 tiles
    ("ataxx7_2x96", "round"),                                      # widened: the zero channels are not returned
    ("chesshist1_1x256_att", "round"),                             # depth 1: the last-layer epilogue alone; two stem chunks
]


def fill(per, workgroups):
    """The smallest batch that gives `workgroups` workgroups of `per` boards."""
    return (workgroups - 1) * per + 1


# network: (family, boards per workgroup of the level, narrow boards per workgroup, workgroups the level must fill)
WIDE = [
    ("chess_2x128_att", "round", 2, 1, T_128),   # 8 tiles
    ("go9_3x128", "weights", 2, 1, T_128),       # 11 tiles
    ("ataxx7_2x128", "round", 4, 2, T_128),      # 13 tiles
    ("chess_2x256_att", "weights", 2, 1, T_256),  # 8 tiles at 256 channels
]
PER_LAYER = [
    ("go19_2x128_conv", "round"),   # one chunk
    ("go19_2x256_conv", "weights"),  # the chunk boundary
    ("go13_2x128_conv", "round"),   # two boards per workgroup
    ("go19_3x192_conv", "round"),   # widened
    ("ataxx7_2x64", "exact"), ("ataxx7_2x64", "round"),  # under one chunk
]


@pytest.fixture(scope="module")
def dev():
    assert capi.device_count() >= 1
    return 0


def built(tables, net, family):
    if family == "exact":
        return tables.build_exact(net, None)
    return tables.build_round(net, None, "round" if family == "weights" else None)


def expected(b):
    """{site: (image or None, stream or None)} from the reference's report, in kz_model_range_site_name's order."""
    depth = b.meta["tower_depth"]
    sites = b.report.sites
    out = {"tower.0": (sites["tower.0"], sites["tower.0.x"])}
    for i in range(1, depth + 1):
        out[f"tower.{i}.mid"] = (sites[f"tower.{i}.mid"], None)
        if i < depth:
            out[f"tower.{i}"] = (sites[f"tower.{i}"], sites[f"tower.{i}.x"])
    out[f"tower.{depth + 1}"] = (None, b.heads.values[f"tower.{depth + 1}"])
    return out


def first_difference(got, want):
    bad = np.argwhere(got != want)
    at = tuple(int(x) for x in bad[0])
    return f"{len(bad)} of {got.size} elements differ, the first at [board, channel, y, x] = {at}: {got[at]} vs {want[at]}"


def check_taps(b, model, image, stream, idx, what):
    want = expected(b)
    assert list(image) == list(stream) == model.range_sites() == list(want), what
    shape = (len(idx), b.meta["tower_channels"], b.meta["board_h"], b.meta["board_w"])
    for site, (q, x) in want.items():
        got_q, got_x = image[site], stream[site]
        assert got_q.shape == got_x.shape == shape and got_q.dtype == np.int8 and got_x.dtype == np.float32
        if q is None:
            assert not got_q.any(), f"{what} {site}: the last site has no image and returns 0"
        else:
            assert not (got_q == -128).any(), f"{what} {site}: {(got_q == -128).sum()} image elements no lane wrote"
            ref = q[idx]
            assert np.array_equal(ref, np.rint(ref)) and np.abs(ref).max() <= 127
            assert np.array_equal(got_q.astype(np.float64), ref), f"{what} {site} image: " + first_difference(got_q.astype(np.float64), ref)
        if x is None:
            assert np.isnan(got_x).all(), f"{what} {site}: a mid site has no stream and returns NaN"
        else:
            assert not np.isnan(got_x).any(), f"{what} {site}: {np.isnan(got_x).sum()} stream elements no lane wrote"
            ref = x[idx]
            assert np.array_equal(got_x.astype(np.float64), ref), f"{what} {site} stream: " + first_difference(got_x.astype(np.float64), ref)


def calibrated(b):
    model = capi.Model(blob=b.blob).quantize_int8(b.site_max)
    assert list(model.int8_site_exponents()) == b.exps[:2 * b.meta["tower_depth"]]
    return model


@pytest.mark.parametrize("net,family", CASES, ids=[f"{n}-{f}" for n, f in CASES])
def test_one_launch_taps_are_the_reference_bits(dev, net, family):
    b = built(N, net, family)
    assert all(b.report.exact.values())
    model = calibrated(b)
    assert model.int8_taps_path(MAX_BATCH, INT8) == "tower_resident_i8"
    hw = b.meta["board_h"] * b.meta["board_w"]
    per = N.boards_per_workgroup(b.meta["tower_channels"], hw)
    assert model.launch_geometry(MAX_BATCH, INT8, N.BOARDS) == ((N.BOARDS + per - 1) // per, per)
    idx = np.arange(N.BOARDS)
    image, stream = model.int8_taps(dev, MAX_BATCH, INT8, b.bits, b.scalars_in)
    check_taps(b, model, image, stream, idx, f"{net} {family}")
    if family != "exact":  # the rounding family clamps at both ends: the taps hold both clamp values
        q0 = image["tower.0"]
        assert (q0 == 127).any() and (q0 == -127).any()
    # dtype 5 returns dtype 4's taps bit for bit (a tap engine never carries heads)
    assert model.int8_taps_path(MAX_BATCH, HEADS) == "tower_resident_i8"
    image5, stream5 = model.int8_taps(dev, MAX_BATCH, HEADS, b.bits, b.scalars_in)
    for site in image:
        assert np.array_equal(image5[site], image[site]) and np.array_equal(stream5[site], stream[site], equal_nan=True), site
    # a range of sites, and one pointer at a time, return the same elements (one board short of the batch: a ragged last workgroup)
    part = idx[:N.BOARDS - 1]
    sites = model.range_sites()
    some_q, some_x = model.int8_taps(dev, MAX_BATCH, INT8, b.bits[part], b.scalars_in[part], site_first=1, n_sites=2)
    assert list(some_q) == sites[1:3]
    for site in some_q:
        assert np.array_equal(some_q[site], image[site][part]) and np.array_equal(some_x[site], stream[site][part], equal_nan=True), site


@pytest.mark.parametrize("net,family,per,narrow,workgroups", WIDE, ids=[f"{w[0]}-{w[1]}" for w in WIDE])
def test_wide_levels_tap_the_reference_bits(dev, net, family, per, narrow, workgroups):
    b = built(N, net, family)
    model = calibrated(b)
    full = per * workgroups
    part = fill(per, workgroups) if per == 2 else full - per + 2  # the last workgroup holds one board of two, two of four
    assert N.boards_per_workgroup(b.meta["tower_channels"], b.meta["board_h"] * b.meta["board_w"]) == narrow
    for n in (full, part):
        assert model.int8_taps_path(full, INT8) == "tower_resident_i8"
        assert model.launch_geometry(full, INT8, n) == (workgroups, per), (net, n)
        assert n % per != 0 or n == full
        idx = np.arange(n) % N.BOARDS
        image, stream = model.int8_taps(dev, full, INT8, b.bits[idx], b.scalars_in[idx])
        check_taps(b, model, image, stream, idx, f"{net} {family}, {n} boards, {per} per workgroup")
    # below the threshold the same engine size taps the narrow tiles, and the bits do not depend on it
    n = fill(per, workgroups) - 1
    assert model.launch_geometry(full, INT8, n) == ((n + narrow - 1) // narrow, narrow)
    idx = np.arange(n) % N.BOARDS
    image, stream = model.int8_taps(dev, full, INT8, b.bits[idx], b.scalars_in[idx], site_first=0, n_sites=2)
    for site in image:
        q, x = expected(b)[site]
        assert np.array_equal(image[site].astype(np.float64), q[idx]), site
        assert x is None or np.array_equal(stream[site].astype(np.float64), x[idx]), site


@pytest.mark.parametrize("net,family", PER_LAYER, ids=[f"{n}-{f}" for n, f in PER_LAYER])
def test_per_layer_taps_are_the_reference_bits(dev, net, family):
    b = built(B, net, family)
    assert all(b.report.exact.values())
    model = calibrated(b)
    assert model.int8_taps_path(MAX_BATCH, ANY) == "board_conv_i8"
    h, w = b.meta["board_h"], b.meta["board_w"]
    assert model.launch_geometry(MAX_BATCH, ANY, B.BOARDS) == (B.workgroups(B.BOARDS, h, w, b.meta["tower_channels"]), 0)
    idx = np.arange(B.BOARDS)
    image, stream = model.int8_taps(dev, MAX_BATCH, ANY, b.bits, b.scalars_in)
    check_taps(b, model, image, stream, idx, f"{net} {family}")
    bpw = B.geometry(h, w)[1]
    part = idx[:bpw + 1]  # a ragged last workgroup
    some_q, some_x = model.int8_taps(dev, MAX_BATCH, ANY, b.bits[part], b.scalars_in[part])
    for site in some_q:
        assert np.array_equal(some_q[site], image[site][part]) and np.array_equal(some_x[site], stream[site][part], equal_nan=True), site


@pytest.mark.parametrize("family", ["exact", "round"])
def test_dtype_8_taps_dtype_5s_tower_where_both_plans_exist(dev, family):
    b = built(N, B.BOTH_PLANS, family)
    model = calibrated(b)
    assert model.int8_taps_path(MAX_BATCH, ANY) == model.int8_taps_path(MAX_BATCH, HEADS) == "tower_resident_i8"
    image8, stream8 = model.int8_taps(dev, MAX_BATCH, ANY, b.bits, b.scalars_in)
    image5, stream5 = model.int8_taps(dev, MAX_BATCH, HEADS, b.bits, b.scalars_in)
    check_taps(b, model, image8, stream8, np.arange(N.BOARDS), f"{B.BOTH_PLANS} {family}, dtype 8")
    for site in image8:
        assert np.array_equal(image8[site], image5[site]) and np.array_equal(stream8[site], stream5[site], equal_nan=True), site
