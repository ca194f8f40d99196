"""kz_model_error_profile: the per-site deviation of the one-launch tower that ships from exact f32, reduced on the device.

On exactly representable networks every arithmetic stores the reference's own bits, so the errors are zero and the reference's
own fields (max |r|, sum r^2, the count) must equal what float64 numpy computes from `report.acts` — the maxima exactly, the sums to
1e-8 relative: at most 2^24 f64 additions of exact squares, an error of n * 2^-53.  On random weights the six fields are recomputed
in numpy float64 from tower_taps(dtype) and tower_taps(F32) of the same boards, and the three arithmetics must come out in the
order of their precision, split16 < f16 < bf16, at every site (they are 2^11 and 2^3 apart: no tuned bound).  One case whose
reference is the per-layer engine (192 channels: no one-launch f32 tower) holds the strided read of its padded NHWC rows; one
with an infinite stem bias holds the non-finite count; one stream-shifted model holds that like is compared with like.
"""
import numpy as np
import pytest

from kzero_amd import capi, synth
from kzero_amd.model_file import read_model, write_model
from tests import exact_nets as E

pytestmark = pytest.mark.gpu

F16, F32, SPLIT, BF16 = capi.KZ_DTYPE_F16, capi.KZ_DTYPE_F32, capi.KZ_DTYPE_F32_SPLIT16, capi.KZ_DTYPE_BF16
NAMES = {F16: "f16", SPLIT: "split16", BF16: "bf16"}
RTOL = 1e-8


@pytest.fixture(scope="module")
def dev():
    assert capi.device_count() >= 1
    return 0


def fields_from(a, r):
    """The six fields in numpy float64 from a site's taps a and its reference r."""
    a, r = a.astype(np.float64), r.astype(np.float64)
    ok = np.isfinite(a) & np.isfinite(r)
    d = a[ok] - r[ok]
    return {"max_abs_err": np.abs(d).max(initial=0.0), "sum_sq_err": float((d * d).sum()), "sum_sq_ref": float((r[ok] * r[ok]).sum()),
            "max_abs_ref": np.abs(r[ok]).max(initial=0.0), "count": int(ok.sum()), "nonfinite": int((~ok).sum())}


def check_fields(row, want, label):
    for f in ("max_abs_err", "max_abs_ref", "count", "nonfinite"):
        assert row[f] == want[f], f"{label} {f}: {row[f]} vs {want[f]}"
    for f in ("sum_sq_err", "sum_sq_ref"):
        assert np.isclose(row[f], want[f], rtol=RTOL, atol=0.0), f"{label} {f}: {row[f]} vs {want[f]}"


@pytest.mark.parametrize("net", ["chess_2x256_att", "ataxx7_1x128"])
@pytest.mark.parametrize("dtype", [F16, SPLIT], ids=["f16", "split16"])
def test_exact_networks_have_no_error_and_the_references_own_fields(dev, net, dtype):
    b = E.build(net, None)
    batch = 9
    model = capi.Model(blob=b.blob)
    prof = model.error_profile(dev, 64, dtype, b.bits[:batch], b.scalars_in[:batch])
    assert list(prof["site"]) == model.range_sites()
    for row in prof:
        r = b.report.acts[row["site"]][:batch]
        assert row["max_abs_err"] == 0 and row["sum_sq_err"] == 0 and row["nonfinite"] == 0, row
        assert row["count"] == r.size == batch * model.info.tower_channels * model.info.board_h * model.info.board_w
        check_fields(row, fields_from(r, r), f"{net} {row['site']}")


@pytest.mark.parametrize("game,depth,channels,head", [("chess", 2, 256, "attention"), ("ataxx-7", 2, 128, "ataxx_conv")], ids=["chess_2x256", "ataxx7_2x128"])
def test_random_weights_match_numpy_and_order_by_precision(dev, game, depth, channels, head):
    model = capi.Model(blob=synth.random_model(game, depth, channels, head, seed=3))
    bits, scalars = synth.random_boards(game, 16, seed=4)
    ref = model.tower_taps(dev, 64, F32, bits, scalars)
    profs = {}
    for dtype in (F16, BF16, SPLIT):
        taps = model.tower_taps(dev, 64, dtype, bits, scalars)
        profs[dtype] = prof = model.error_profile(dev, 64, dtype, bits, scalars)
        for row in prof:
            want = fields_from(taps[row["site"]], ref[row["site"]])
            assert want["count"] == 16 * channels * model.info.board_h * model.info.board_w and want["nonfinite"] == 0
            check_fields(row, want, f"{game} {NAMES[dtype]} {row['site']}")
            rel = np.sqrt(row["sum_sq_err"] / row["sum_sq_ref"])
            print(f"[error profile] {game} {depth}x{channels} {NAMES[dtype]:>7} {row['site']:<12} max|err| {row['max_abs_err']:.4g}  "
                  f"rms/rms {rel:.3g}  max|ref| {row['max_abs_ref']:.4g}")
    for i, site in enumerate(model.range_sites()):
        s, h, bf = (profs[d][i]["sum_sq_err"] for d in (SPLIT, F16, BF16))
        assert s < h < bf, f"{site}: sum_sq_err split16 {s} f16 {h} bf16 {bf}"


def test_the_per_layer_reference_reads_its_padded_rows(dev):
    """192 channels: no one-launch f32 tower, the reference is the per-layer exact-f32 engine (rows of 192 floats in this case;
    the kernel takes the stride as an argument)."""
    b = E.build("chess_1x192_att", None)
    model = capi.Model(blob=b.blob)
    assert model.range_profile_fast_path() == "conv_igemm_f32"
    batch = 9
    prof = model.error_profile(dev, 64, F16, b.bits[:batch], b.scalars_in[:batch])
    for row in prof:
        r = b.report.acts[row["site"]][:batch]
        assert row["max_abs_err"] == 0 and row["sum_sq_err"] == 0 and row["nonfinite"] == 0, row
        assert row["count"] == batch * 192 * 64
        check_fields(row, fields_from(r, r), row["site"])


def test_channels_that_are_no_multiple_of_32_compare_the_real_ones(dev):
    """48 tower channels run widened to 64 in f16; the per-layer reference has rows padded to 64 floats: the 48 real channels
    are compared, the padding is not."""
    b = E.build("ataxx7_1x48", None)
    model = capi.Model(blob=b.blob)
    assert model.tower_taps_path(64, F16) == "tower_resident_f16g"
    batch = 5
    taps = model.tower_taps(dev, 64, F16, b.bits[:batch], b.scalars_in[:batch])
    prof = model.error_profile(dev, 64, F16, b.bits[:batch], b.scalars_in[:batch])
    for row in prof:
        r = b.report.acts[row["site"]][:batch]
        assert np.array_equal(taps[row["site"]], r.astype(np.float32)), row["site"]
        assert row["max_abs_err"] == 0 and row["nonfinite"] == 0 and row["count"] == batch * 48 * 49, row
        check_fields(row, fields_from(r, r), row["site"])


def test_a_non_finite_site_is_counted_and_left_out(dev):
    meta, t = read_model(synth.random_model("chess", 2, 256, "attention", seed=3))
    t["common.tower.0.bias"] = t["common.tower.0.bias"].copy()
    t["common.tower.0.bias"][5] = np.inf
    model = capi.Model(blob=write_model(meta, t))
    bits, scalars = synth.random_boards("chess", 16, seed=4)
    prof = model.error_profile(dev, 64, F16, bits, scalars)  # (returns: the call does not fail on a non-finite network)
    ref = model.tower_taps(dev, 64, F32, bits, scalars)
    taps = model.tower_taps(dev, 64, F16, bits, scalars)
    for row in prof:
        assert row["nonfinite"] > 0, row
        assert all(np.isfinite(row[f]) for f in ("max_abs_err", "sum_sq_err", "sum_sq_ref", "max_abs_ref")), row
        assert row["count"] + row["nonfinite"] == 16 * 256 * 64
        want = fields_from(taps[row["site"]], ref[row["site"]])
        check_fields(row, want, row["site"])
    assert prof[0]["nonfinite"] == 16 * 64, "the stem's channel 5 on every square of every board"


def test_a_stream_shifted_model_compares_like_with_like(dev):
    b = E.build("chess_2x256_att", None)
    model = capi.Model(blob=b.blob)
    batch = 9
    base = model.error_profile(dev, 64, F16, b.bits[:batch], b.scalars_in[:batch])
    shifted = model.stream_shift(4).error_profile(dev, 64, F16, b.bits[:batch], b.scalars_in[:batch])
    n = len(base)
    for i in range(n):
        assert shifted[i]["max_abs_err"] == 0 and shifted[i]["nonfinite"] == 0 and shifted[i]["count"] == base[i]["count"]
        unit = 2.0 ** -4 if i < n - 1 else 1.0  # (the last site is behind the final BN: a shift does not move it)
        assert shifted[i]["max_abs_ref"] == base[i]["max_abs_ref"] * unit, (i, shifted[i], base[i])
