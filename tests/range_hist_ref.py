"""What the range histogram's tests share (tests/test_range_histogram.py, test_range_histogram_cpp.py,
test_gpu_range_histogram.py): the bins restated from the definition in include/kz_hip.h, crafted histograms, and a numpy
restatement of the bindings' shift_report."""
import os

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "kz_hip.h")
BINS = 96
FIELDS = ("total", "zero", "nonfinite", "f16_over", "f16_top", "f16_subnormal", "f16_flushed", "split_lo_subnormal",
          "clamped_low", "clamped_high")
REPORT_KS = (-24, 0, 3, 24)


def bin_of(x):
    """The bin of every f32 value of x, from the header's definition: integer arithmetic on the bit pattern."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    a = u & np.uint32(0x7fffffff)
    e = (a >> np.uint32(23)).astype(np.int64)
    big_e = e - 127  # (an f32 subnormal, e = 0, counts as E = -127: the clamp takes it to -50 like every E below)
    b = np.clip(big_e, -50, 43) + 51
    b = np.where(e == 255, 95, b)
    return np.where(a == 0, 0, b).astype(np.int64)


def histogram_of(x):
    """uint64 [96]: the counts of all elements of x."""
    return np.bincount(bin_of(x).ravel(), minlength=BINS).astype(np.uint64)


def shift_bins(hist, k):
    """hist [n_sites, 96] as a stream 2^-k times as large has it: the binade bins of the shifted sites (all but the last) moved
    down by k, the two end bins absorbing what leaves 2 .. 93; zeros and non-finite values stay where they are."""
    hist = np.asarray(hist, np.uint64)
    out = hist.copy()
    for site in range(hist.shape[0] - 1):
        row = np.zeros(BINS, np.uint64)
        row[0], row[95] = hist[site, 0], hist[site, 95]
        for b in range(1, 95):
            row[min(max(b - k, 1), 94)] += hist[site, b]
        out[site] = row
    return out


def shift_report_ref(hist, k):
    """The counts of capi.shift_report, with numpy masks over the exponent of each bin."""
    hist = np.asarray(hist, np.uint64)
    n = hist.shape[0]
    shift = np.full(n, k)
    shift[-1] = 0
    e = (np.arange(BINS) - 51)[None, :] - shift[:, None]  # E' of bin b at each site
    real = np.zeros(BINS, bool)
    real[1:95] = True

    def count(mask):
        return (hist * (mask & real[None, :])).sum(axis=1).astype(np.uint64)

    return {"total": hist.sum(axis=1).astype(np.uint64), "zero": hist[:, 0].copy(), "nonfinite": hist[:, 95].copy(),
            "f16_over": count(e >= 16), "f16_top": count(e == 15), "f16_subnormal": count((e >= -25) & (e <= -15)),
            "f16_flushed": count(e < -25), "split_lo_subnormal": count(e <= -3),
            "clamped_low": hist[:, 1].copy(), "clamped_high": hist[:, 94].copy()}


def crafted_tables():
    """Histograms with every class non-empty under every k of REPORT_KS, the end bins included."""
    rng = np.random.default_rng(11)
    every_bin = rng.integers(1, 1000, size=(5, BINS)).astype(np.uint64)  # every bin of every site holds something
    large = np.zeros((3, BINS), np.uint64)
    large[:, :] = np.arange(BINS, dtype=np.uint64)[None, :] * np.uint64(1 << 33) + np.uint64(7)  # counts beyond 2^32
    single = rng.integers(1, 50, size=(1, BINS)).astype(np.uint64)  # one site: it is the last one, unshifted
    ends = np.zeros((2, BINS), np.uint64)
    ends[:, [0, 1, 94, 95]] = [[1, 2, 3, 4], [5, 6, 7, 8]]  # nothing but zeros, the end bins and non-finite values
    return {"every_bin": every_bin, "large": large, "single": single, "ends": ends}
