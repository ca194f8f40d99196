"""The range histogram without a GPU (include/kz_hip.h, "range histogram"): the bins, restated here from the header's
definition and held to known answers; capi.shift_report against a numpy restatement on crafted histograms; and the two entries,
which fail loudly and in their own name where there is no device.

tests/range_hist_ref.py holds what the GPU test and the C++ test share: bin_of, the crafted tables and the restatement."""
import numpy as np
import pytest

from kzero_amd import capi, synth
from tests import range_hist_ref as R


def f32(x):
    return np.array([x], np.float32)


def below(x):
    return np.nextafter(np.float32(x), np.float32(0))


def test_bins_is_the_headers_number():
    assert capi.KZ_RANGE_BINS == R.BINS == 96
    text = open(R.HEADER).read()
    assert "#define KZ_RANGE_BINS 96" in text


@pytest.mark.parametrize("value, want", [
    (0.0, 0), (-0.0, 0),
    (2.0 ** -149, 1),                                   # the smallest f32 subnormal: E counts as -127
    (np.float32(2.0 ** -126) - np.float32(2.0 ** -149), 1),  # the largest f32 subnormal
    (2.0 ** -126, 1),
    (2.0 ** -50, 1), (below(2.0 ** -49), 1), (2.0 ** -49, 2),
    (1.0, 51), (-1.0, 51), (below(1.0), 50), (1.5, 51),
    (65504.0, 66), (65536.0, 67),
    (below(2.0 ** 43), 93), (2.0 ** 43, 94), (-2.0 ** 43, 94),
    (np.finfo(np.float32).max, 94),
    (np.inf, 95), (-np.inf, 95), (np.nan, 95), (-np.nan, 95),
])
def test_bin_of_known_answers(value, want):
    assert int(R.bin_of(f32(value))[0]) == want


def test_bin_of_window_and_every_exponent():
    # f16's whole window under every k in [-24, 24]: 2^-25 at k = -24 is bin 2, 2^16 at k = 24 is bin 91
    assert int(R.bin_of(f32(2.0 ** (-25 - 24)))[0]) == 2 and int(R.bin_of(f32(2.0 ** (16 + 24)))[0]) == 91
    # every biased exponent, both signs, the smallest and the largest mantissa of each
    e = np.arange(256, dtype=np.uint32)
    for mant in (0, 0x7fffff):
        for sign in (0, 0x80000000):
            u = (e << 23 | mant | sign).astype(np.uint32)
            got = R.bin_of(u.view(np.float32))
            want = np.clip(e.astype(int) - 127, -50, 43) + 51
            want[255] = 95
            if mant == 0:
                want[0] = 0
            assert np.array_equal(got, want), (mant, sign)
    # bin b in 2 .. 93 holds 2^(b-51) <= |x| < 2^(b-50)
    for b in range(2, 94):
        lo, hi = np.float32(2.0 ** (b - 51)), np.float32(2.0 ** (b - 50))
        assert int(R.bin_of(f32(lo))[0]) == b and int(R.bin_of(f32(below(hi)))[0]) == b


def test_histogram_of_counts_every_element_once():
    rng = np.random.default_rng(1)
    x = (rng.standard_normal(5000) * 10.0 ** rng.integers(-20, 20, 5000)).astype(np.float32)
    x[::7] = 0
    x[5], x[6] = np.inf, np.nan
    h = R.histogram_of(x)
    assert h.dtype == np.uint64 and h.shape == (96,) and int(h.sum()) == x.size
    assert h[0] == (x == 0).sum() and h[95] == 2


@pytest.mark.parametrize("k", R.REPORT_KS)
@pytest.mark.parametrize("table", sorted(R.crafted_tables()))
def test_shift_report_against_the_restatement(table, k):
    hist = R.crafted_tables()[table]
    got, want = capi.shift_report(hist, k), R.shift_report_ref(hist, k)
    assert tuple(got) == capi.SHIFT_REPORT_FIELDS == R.FIELDS
    for name in R.FIELDS:
        assert got[name].dtype == np.uint64 and got[name].shape == (hist.shape[0],)
        assert np.array_equal(got[name], want[name]), (name, got[name], want[name])
    assert np.array_equal(got["total"], hist.sum(axis=1))


def test_shift_report_known_numbers():
    """One value per class, by hand: three sites, the last unshifted."""
    hist = np.zeros((3, 96), np.uint64)
    hist[:, 0], hist[:, 95] = 5, 2                      # zeros and non-finite: in no class
    hist[:, 1], hist[:, 94] = 3, 4                      # the clamped end bins
    hist[:, 51 + 15] = 10                               # E = 15
    hist[:, 51 + 18] = 20                               # E = 18
    hist[:, 51 - 12] = 30                               # E = -12
    hist[:, 51 - 23] = 40                               # E = -23
    hist[:, 51] = 50                                    # E = 0
    total = 5 + 2 + 3 + 4 + 10 + 20 + 30 + 40 + 50
    r = capi.shift_report(hist, 3)
    # shifted sites: E' = 12, 15, -15, -26, -3; last site: E' = E
    for name, want in [("total", [total] * 3), ("zero", [5] * 3), ("nonfinite", [2] * 3),
                       ("f16_over", [4, 4, 4 + 20]), ("f16_top", [20, 20, 10]),
                       ("f16_subnormal", [30, 30, 40]), ("f16_flushed", [3 + 40, 3 + 40, 3]),
                       ("split_lo_subnormal", [3 + 30 + 40 + 50, 3 + 30 + 40 + 50, 3 + 30 + 40]),
                       ("clamped_low", [3] * 3), ("clamped_high", [4] * 3)]:
        assert r[name].tolist() == want, name
    # the end bins stay in their class for every k the shift takes
    for k in (-24, 24):
        r = capi.shift_report(hist, k)
        assert (r["f16_flushed"] >= r["clamped_low"]).all() and (r["f16_over"] >= r["clamped_high"]).all()
        assert (r["split_lo_subnormal"] >= r["clamped_low"]).all()


def test_shift_report_refuses_what_it_cannot_read():
    hist = np.zeros((3, 96), np.uint64)
    for bad in (np.zeros((3, 95), np.uint64), np.zeros(96, np.uint64), np.zeros((0, 96), np.uint64)):
        with pytest.raises(capi.KzError, match="shift_report"):
            capi.shift_report(bad, 0)
    for k in (-25, 25):
        with pytest.raises(capi.KzError, match="shift_report: k = "):
            capi.shift_report(hist, k)


@pytest.mark.parametrize("fast, fn", [(True, "kz_model_range_histogram_fast"), (False, "kz_model_range_histogram")])
def test_the_entries_check_their_arguments_and_fail_in_their_own_name(fast, fn):
    """Argument checks come before any device call; and where no device is visible the call fails with a message, in its own
    name (with one it succeeds: tests/test_gpu_range_histogram.py)."""
    model = capi.Model(blob=synth.random_model("ataxx-7", 2, 16, "ataxx_conv", seed=1))
    bits, scalars = synth.random_boards("ataxx-7", 3, seed=1)
    with pytest.raises(capi.KzError) as e:
        model.range_histogram(0, bits[:, :-1], scalars, fast=fast)
    assert str(e.value) == f"{fn}: bits_stride too small"
    with pytest.raises(capi.KzError) as e:
        model.range_histogram(0, bits[:0], scalars[:0], fast=fast)
    assert str(e.value) == f"{fn}: batch must be positive"
    try:
        gpus = capi.device_count()
    except capi.KzError:
        gpus = 0
    if gpus == 0:
        with pytest.raises(capi.KzError) as e:
            model.range_histogram(0, bits, scalars, fast=fast)
        assert str(e.value).startswith(fn + ": ") and "KZ_" not in str(e.value), str(e.value)
