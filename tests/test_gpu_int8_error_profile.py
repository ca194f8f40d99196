"""kz_model_int8_error_profile on the GPU: per range site the deviation of the stored int8 image (q * 2^e_s) and of the f16 stream
value beside it from exact f32, with the two clamp counts, reduced on the device.

Against the reference's report (tests/int8_nets.py, tests/int8_board_nets.py; exact and rounding families, one one-launch and one
per-layer network): at_clamp is (|q| == 127).sum() of `report.sites`, the exponents are the calibration's, and in the exact family
— where the int8 reference equals the unquantised one — the image has no error at all.

Against numpy on random weights (synth.random_model; chess 2x256, Ataxx-7 2x128, Go-19 2x128 at 16 boards, calibrated on the
evaluated boards with headroom 1): both kz_site_error records are recomputed in float64 from int8_taps and the exact-f32 tensors of
the same boards — tower_taps(F32), or for the per-layer shape the exact-f32 engine's kept activations —, the maxima and the counts
exactly, the sums to the 1e-8 relative of tests/test_gpu_error_profile.py (derived there: at most 2^24 f64 additions of exact
squares).  With headroom 1, 127 * 2^e_s >= site_max, so no reference value lies beyond 127.5 steps: ref_beyond == 0 at every
site.  Recalibrated with every site maximum x 0.25 the exponent is e_s - 2, and 127.5 * 2^(e_s - 2) < site_max follows from the
definition of the ceiling (127 * 2^(e_s - 1) < site_max): the site's largest value lies beyond, ref_beyond >= 1 at every quantised
site.  And an image of seven bits is further from exact f32 than the f16 engine's eleven: its sum_sq_err is above the f16 engine's
at every quantised site, on the same boards (kz_model_error_profile where that engine runs one launch; for Go 19x19, which it
runs per layer, the same sum in numpy from the f16 engine's kept activations).  No tuned bound.

Never-written detection: with a part-filled last workgroup the counts cover batch * C * H * W elements and image.nonfinite == 0
(the image part of the tap buffer is 0x80 before every pass, and -128 counts as non-finite)."""
import numpy as np
import pytest

from kzero_amd import capi, synth
from tests import int8_board_nets as B
from tests import int8_nets as N
from tests.test_gpu_error_profile import RTOL, check_fields, fields_from

pytestmark = pytest.mark.gpu

INT8, HEADS, ANY = capi.KZ_DTYPE_INT8, capi.KZ_DTYPE_INT8_HEADS, capi.KZ_DTYPE_INT8_ANY
F16, F32 = capi.KZ_DTYPE_F16, capi.KZ_DTYPE_F32
MAX_BATCH = 64
REPORT_CASES = [(N, "ataxx7_2x128", INT8, "tower_resident_i8"), (B, "go13_2x128_conv", ANY, "board_conv_i8")]
RANDOM = [("chess", 2, 256, "attention", INT8), ("ataxx-7", 2, 128, "ataxx_conv", INT8), ("go-19", 2, 128, "conv", ANY)]
assert RTOL == 1e-8


@pytest.fixture(scope="module")
def dev():
    assert capi.device_count() >= 1
    return 0


def site_kinds(n):
    """(sites with an image, sites with a stream) of n range sites: all but the last; the stem, the block outputs and the last."""
    return list(range(n - 1)), list(range(0, n, 2))


def elements(model, batch):
    return batch * model.info.tower_channels * model.info.board_h * model.info.board_w


@pytest.mark.parametrize("family", ["exact", "round"])
@pytest.mark.parametrize("tables,net,dtype,path", REPORT_CASES, ids=[c[1] for c in REPORT_CASES])
def test_clamp_counts_and_exponents_are_the_reports(dev, tables, net, dtype, path, family):
    b = tables.build_exact(net, None) if family == "exact" else tables.build_round(net, None)
    model = capi.Model(blob=b.blob).quantize_int8(b.site_max)
    assert model.int8_taps_path(MAX_BATCH, dtype) == path
    prof = model.int8_error_profile(dev, MAX_BATCH, dtype, b.bits, b.scalars_in)
    names = model.range_sites()
    assert list(prof["site"]) == names and len(prof) == 2 * b.meta["tower_depth"] + 1
    total = elements(model, len(b.bits))
    images, streams = site_kinds(len(names))
    for i, row in enumerate(prof):
        print(f"[int8 error profile] {net} {family} {row['site']:<12} e {row['exponent']:>3} at_clamp {row['at_clamp']:>7} ref_beyond {row['ref_beyond']:>7} "
              f"image max|err| {row['image']['max_abs_err']:.4g} stream max|err| {row['stream']['max_abs_err']:.4g}")
        assert row["reserved"] == 0
        if i in images:
            q = b.report.sites[row["site"]]
            assert row["at_clamp"] == int((np.abs(q) == 127).sum()), row["site"]
            assert row["exponent"] == b.exps[i], row["site"]
            assert row["image"]["nonfinite"] == 0 and row["image"]["count"] == total == q.size
        else:
            assert row["at_clamp"] == row["ref_beyond"] == row["exponent"] == 0 and row["image"]["count"] == row["image"]["nonfinite"] == 0
        assert row["stream"]["count"] == (total if i in streams else 0) and row["stream"]["nonfinite"] == 0
        if family == "exact":  # nothing rounds, nothing clamps: the int8 reference is the unquantised one
            assert row["image"]["sum_sq_err"] == 0 and row["image"]["max_abs_err"] == 0, row
            assert row["stream"]["sum_sq_err"] == 0 and row["stream"]["max_abs_err"] == 0, row
            assert row["ref_beyond"] == 0
    if family == "round":  # the family with clamps at both ends: the counts are not trivially zero
        assert all(prof[i]["at_clamp"] > 0 for i in images), prof["at_clamp"]
        assert prof[0]["ref_beyond"] > 0


def exact_f32_sites(model, dev, bits, scalars, monkeypatch):
    """{site: float32 [batch, C, H, W]} of the exact network on these boards: the one-launch f32 tower's taps, or for a shape that
    tower does not take the per-layer exact-f32 engine's kept activations."""
    if model.range_profile_fast_path() == "tower_resident_f32":
        return model.tower_taps(dev, len(bits), F32, bits, scalars)
    return kept_activations(model, dev, F32, bits, scalars, monkeypatch)


def kept_activations(model, dev, dtype, bits, scalars, monkeypatch):
    monkeypatch.setenv("KZ_KEEP_ACTIVATIONS", "1")
    try:
        eng = capi.Engine(model, dev, len(bits), dtype)
        assert eng.tower_path.startswith("conv_igemm"), eng.tower_path
        eng.eval_packed(bits, scalars)
        return {site: eng.read_activation(site, len(bits)) for site in model.range_sites()}
    finally:
        monkeypatch.delenv("KZ_KEEP_ACTIVATIONS")


@pytest.mark.parametrize("game,depth,channels,head,dtype", RANDOM, ids=[f"{r[0]}_{r[1]}x{r[2]}" for r in RANDOM])
def test_random_weights_match_numpy(dev, game, depth, channels, head, dtype, monkeypatch):
    batch = 16
    plain = capi.Model(blob=synth.random_model(game, depth, channels, head, seed=3))
    bits, scalars = synth.random_boards(game, batch, seed=4)
    site_max, _ = plain.range_profile_fast(dev, bits, scalars)
    model = plain.quantize_int8(site_max.astype(np.float64))  # headroom 1 on the evaluated boards (capi.calibrate_int8)
    exps = model.int8_site_exponents()
    names = model.range_sites()
    images, streams = site_kinds(len(names))
    ref = exact_f32_sites(model, dev, bits, scalars, monkeypatch)
    image, stream = model.int8_taps(dev, batch, dtype, bits, scalars)
    prof = model.int8_error_profile(dev, batch, dtype, bits, scalars)
    total = elements(model, batch)
    empty = fields_from(np.zeros(0), np.zeros(0))
    for i, row in enumerate(prof):
        site, r = row["site"], ref[row["site"]]
        assert np.abs(r).max() == site_max[i], f"{site}: the reference is the tensor the calibration measured"
        if i in images:
            q = image[site]
            assert not (q == -128).any()
            a = q.astype(np.float64) * 2.0 ** int(exps[i])
            want = fields_from(a, r)
            assert want["count"] == total and want["nonfinite"] == 0
            check_fields(row["image"], want, f"{game} {site} image")
            assert row["at_clamp"] == int((np.abs(q.astype(np.int32)) == 127).sum()) and row["exponent"] == exps[i]
            beyond = int((np.isfinite(r) & (np.abs(r).astype(np.float32) * np.float32(2.0 ** -int(exps[i])) >= np.float32(127.5))).sum())
            assert row["ref_beyond"] == beyond == 0, f"{site}: headroom 1 leaves no reference value beyond 127.5 steps"
        else:
            check_fields(row["image"], empty, f"{game} {site} image")
            assert row["at_clamp"] == row["ref_beyond"] == row["exponent"] == 0
        if i in streams:
            want = fields_from(stream[site], r)
            assert want["count"] == total and want["nonfinite"] == 0
            check_fields(row["stream"], want, f"{game} {site} stream")
        else:
            assert np.isnan(stream[site]).all()
            check_fields(row["stream"], empty, f"{game} {site} stream")
        rel = lambda part: np.sqrt(part["sum_sq_err"] / part["sum_sq_ref"]) if part["count"] else float("nan")  # noqa: E731
        print(f"[int8 error profile] {game} {depth}x{channels} {site:<12} e {row['exponent']:>3} image rms/rms {rel(row['image']):.3g} max|err| "
              f"{row['image']['max_abs_err']:.4g}  stream rms/rms {rel(row['stream']):.3g}  at_clamp {row['at_clamp']}  ref_beyond {row['ref_beyond']}")

    # seven bits against eleven: the image is further from exact f32 than the f16 engine's stored tensor of the same site
    if plain.range_profile_fast_path() == "tower_resident_f32":
        f16_err = plain.error_profile(dev, batch, F16, bits, scalars)["sum_sq_err"]
    else:  # (Go 19x19: the f16 engine runs per layer, where kz_model_error_profile has no taps — its kept activations instead)
        kept = kept_activations(plain, dev, F16, bits, scalars, monkeypatch)
        f16_err = [fields_from(kept[site], ref[site])["sum_sq_err"] for site in names]
    for i in images:
        assert prof[i]["image"]["sum_sq_err"] > f16_err[i], f"{names[i]}: int8 image {prof[i]['image']['sum_sq_err']} vs f16 {f16_err[i]}"

    # every site maximum x 0.25: the exponent drops by two and the site's largest value lies beyond 127.5 steps
    tight = plain.quantize_int8(site_max.astype(np.float64) * 0.25)
    assert list(tight.int8_site_exponents()) == [int(e) - 2 for e in exps]
    tight_prof = tight.int8_error_profile(dev, batch, dtype, bits, scalars)
    for i in images:
        assert tight_prof[i]["ref_beyond"] >= 1, tight_prof[i]
        assert tight_prof[i]["exponent"] == exps[i] - 2
    assert tight_prof[-1]["ref_beyond"] == 0 and tight_prof[-1]["at_clamp"] == 0


@pytest.mark.parametrize("tables,net,dtype,batch", [(N, "ataxx7_2x128", INT8, 13), (N, "chess_2x256_att", HEADS, 7), (B, "go13_2x128_conv", ANY, 5)],
                         ids=["ataxx7_2x128", "chess_2x256_att", "go13_2x128_conv"])
def test_a_part_filled_last_workgroup_leaves_nothing_unwritten(dev, tables, net, dtype, batch):
    """Two boards per workgroup and an odd batch (the one-launch tower's seven tiles, the per-layer kernel on 13x13), and one board
    per workgroup at 256 channels as the plain case: every element of every real board is counted, none as never written."""
    b = tables.build_round(net, None)
    model = capi.Model(blob=b.blob).quantize_int8(b.site_max)
    wgs, per = model.launch_geometry(MAX_BATCH, dtype if dtype != HEADS else INT8, batch)
    if net != "chess_2x256_att":
        bpw = per if per else B.geometry(b.meta["board_h"], b.meta["board_w"])[1]
        assert bpw == 2 and batch % 2 == 1
    prof = model.int8_error_profile(dev, MAX_BATCH, dtype, b.bits[:batch], b.scalars_in[:batch])
    total = elements(model, batch)
    images, streams = site_kinds(len(prof))
    for i, row in enumerate(prof):
        assert row["image"]["nonfinite"] == 0 and row["stream"]["nonfinite"] == 0, row
        assert row["image"]["count"] == (total if i in images else 0), row
        assert row["stream"]["count"] == (total if i in streams else 0), row
        if i in images:
            q = b.report.sites[row["site"]][:batch]
            assert row["at_clamp"] == int((np.abs(q) == 127).sum())


def test_a_profile_in_two_chunks_is_the_sum_of_its_parts(dev):
    """The per-layer reference takes at most 64 boards at a time: 70 boards of Go 19x19 go through as 64 + 6.  The counts of the
    whole are the sums of the two parts' and the maxima their maxima, exactly; the f64 sums add up to the 1e-8 relative above."""
    plain = capi.Model(blob=synth.random_model("go-19", 1, 128, "conv", seed=3))
    bits, scalars = synth.random_boards("go-19", 70, seed=4)
    model = capi.calibrate_int8(plain, dev, bits[:16], scalars[:16], headroom=1.0)
    assert model.int8_taps_path(128, ANY) == "board_conv_i8" and model.range_profile_fast_path() == "conv_igemm_f32"
    whole = model.int8_error_profile(dev, 128, ANY, bits, scalars)
    parts = [model.int8_error_profile(dev, 128, ANY, bits[lo:hi], scalars[lo:hi]) for lo, hi in ((0, 64), (64, 70))]
    for i, row in enumerate(whole):
        for f in ("at_clamp", "ref_beyond"):
            assert row[f] == sum(p[i][f] for p in parts), (row["site"], f)
        assert row["exponent"] == parts[0][i]["exponent"] == parts[1][i]["exponent"]
        for rec in ("image", "stream"):
            for f in ("count", "nonfinite"):
                assert row[rec][f] == sum(p[i][rec][f] for p in parts), (row["site"], rec, f)
            for f in ("max_abs_err", "max_abs_ref"):
                assert row[rec][f] == max(p[i][rec][f] for p in parts), (row["site"], rec, f)
            for f in ("sum_sq_err", "sum_sq_ref"):
                assert np.isclose(row[rec][f], sum(p[i][rec][f] for p in parts), rtol=RTOL, atol=0.0), (row["site"], rec, f)
    assert whole[0]["image"]["count"] == elements(model, 70) and whole[0]["image"]["nonfinite"] == 0
