// test_range_histogram.cpp — the C++ mirror's shift_report (kzero_amd/csrc/host/hip_network.hpp) on the crafted histograms of
// tests/range_hist_ref.py, with the numbers its numpy restatement gives; the hand-made table of tests/test_range_histogram.py;
// the refusals; and, without a device, the two entries' failure in their own name.  Needs no GPU.
// usage: test_range_histogram <cases.txt> <model.kzm>
//   cases.txt: per case "case <name> <n_sites> <k>", then n_sites lines of 96 counts, then n_sites lines of the ten expected
//   counts in ShiftReport's order
#include <cstdio>
#include <fstream>
#include <stdexcept>
#include <string>

#include "../../kzero_amd/csrc/host/hip_network.hpp"

using namespace kz::host;

static int failures = 0;
#define CHECK(cond)                                                \
    do {                                                           \
        if (!(cond)) {                                             \
            failures++;                                            \
            printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
        }                                                          \
    } while (0)

static std::vector<uint64_t> fields(const ShiftReport &r) {
    return {r.total, r.zero, r.nonfinite, r.f16_over, r.f16_top, r.f16_subnormal, r.f16_flushed, r.split_lo_subnormal,
            r.clamped_low, r.clamped_high};
}

template <class F>
static bool throws_invalid(F &&f) {
    try {
        f();
    } catch (const std::invalid_argument &) {
        return true;
    }
    return false;
}

int main(int argc, char **argv) {
    if (argc < 3) return 2;
    static_assert(KZ_RANGE_BINS == 96, "the header's bins");
    std::ifstream in(argv[1]);
    std::string word, name;
    int cases = 0;
    while (in >> word) {
        size_t n = 0;
        int k = 0;
        if (word != "case" || !(in >> name >> n >> k)) return 2;
        std::vector<uint64_t> hist(n * KZ_RANGE_BINS);
        for (auto &v : hist) in >> v;
        std::vector<uint64_t> want(n * 10);
        for (auto &v : want) in >> v;
        if (!in) return 2;
        const std::vector<ShiftReport> got = shift_report(hist, k);
        CHECK(got.size() == n);
        for (size_t site = 0; site < n && site < got.size(); site++) {
            const std::vector<uint64_t> f = fields(got[site]);
            for (size_t j = 0; j < 10; j++)
                if (f[j] != want[site * 10 + j]) {
                    failures++;
                    printf("FAIL %s k %d site %zu field %zu: %llu, expected %llu\n", name.c_str(), k, site, j, (unsigned long long)f[j],
                           (unsigned long long)want[site * 10 + j]);
                }
        }
        cases++;
    }
    CHECK(cases >= 16);

    // one value per class, by hand: three sites, the last unshifted (tests/test_range_histogram.py)
    {
        std::vector<uint64_t> hist(3 * KZ_RANGE_BINS, 0);
        for (int s = 0; s < 3; s++) {
            uint64_t *row = hist.data() + s * KZ_RANGE_BINS;
            row[0] = 5, row[95] = 2, row[1] = 3, row[94] = 4;
            row[51 + 15] = 10, row[51 + 18] = 20, row[51 - 12] = 30, row[51 - 23] = 40, row[51] = 50;
        }
        const auto r = shift_report(hist, 3);
        const uint64_t total = 5 + 2 + 3 + 4 + 10 + 20 + 30 + 40 + 50;
        CHECK(fields(r[0]) == (std::vector<uint64_t>{total, 5, 2, 4, 20, 30, 43, 123, 3, 4}));
        CHECK(fields(r[1]) == fields(r[0]));
        CHECK(fields(r[2]) == (std::vector<uint64_t>{total, 5, 2, 24, 10, 40, 3, 73, 3, 4}));
        CHECK(throws_invalid([&] { shift_report(hist, 25); }) && throws_invalid([&] { shift_report(hist, -25); }));
        hist.pop_back();
        CHECK(throws_invalid([&] { shift_report(hist, 0); }));
        CHECK(throws_invalid([&] { shift_report(std::vector<uint64_t>(), 0); }));
    }

    // the entries through HipModel: argument checks in their own name; without a device the call itself fails in its name
    HipModel model{std::string(argv[2])};
    const std::vector<uint8_t> bits((size_t)model.info.bits_bytes, 0);
    const std::vector<float> scalars((size_t)std::max(model.info.input_scalar_channels, 1), 0.0f);
    for (const bool fast : {true, false}) {
        const std::string fn = fast ? "kzhip: kz_model_range_histogram_fast: " : "kzhip: kz_model_range_histogram: ";
        std::string what;
        try {
            model.range_histogram(0, bits.data(), bits.size(), scalars.data(), 0, fast);
        } catch (const std::runtime_error &e) {
            what = e.what();
        }
        CHECK(what == fn + "batch must be positive");
        int gpus = 0;
        if (kz_device_count(&gpus) != 0) gpus = 0;
        if (gpus == 0) {
            what.clear();
            try {
                model.range_histogram(0, bits.data(), bits.size(), scalars.data(), 1, fast);
            } catch (const std::runtime_error &e) {
                what = e.what();
            }
            CHECK(what.rfind(fn, 0) == 0 && what.find("KZ_") == std::string::npos);
        }
    }
    if (failures) return 1;
    printf("range histogram tests ok: %d cases\n", cases);
    return 0;
}
