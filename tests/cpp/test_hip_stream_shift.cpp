// test_hip_stream_shift.cpp — the C++ mirror's side of the stream shift (kzero_amd/csrc/host/hip_network.hpp): shift_for against
// the rule's table, HipModel::stream_shift / range_sites through the C ABI.  Needs no GPU.  usage: test_hip_stream_shift <model.kzm>
#include <cstdio>
#include <stdexcept>

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

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    // k = max(0, ceil(log2(m / 65504)) + headroom_bits)
    const struct { float m; int headroom, k; } table[] = {
        {65504.0f, 0, 0}, {65504.0f, 2, 2}, {65505.0f, 0, 1}, {65505.0f, 2, 3}, {1.0f, 0, 0}, {1.0f, 2, 0}, {0.0f, 2, 0},
        {2 * 65504.0f, 0, 1}, {2 * 65504.0f + 16, 0, 2}, {1.0e6f, 0, 4}, {1.0e6f, 2, 6}, {32752.0f, 2, 1}, {32754.0f, 2, 2},
        {16376.0f, 2, 0}, {65504.0f * 4096, 2, 14},
    };
    for (const auto &row : table) CHECK(shift_for(row.m, row.headroom) == row.k);
    CHECK(shift_for(65505.0f) == 3);  // two bits by default
    bool threw = false;
    try {
        shift_for(-1.0f, 0);
    } catch (const std::invalid_argument &) {
        threw = true;
    }
    CHECK(threw);

    HipModel model{std::string(argv[1])};
    const auto sites = model.range_sites();
    CHECK((int)sites.size() == 2 * model.info.tower_depth + 1);
    CHECK(sites.front() == "tower.0" && sites.back() == "tower." + std::to_string(model.info.tower_depth + 1));
    CHECK(sites.size() < 2 || sites[1] == "tower.1.mid");
    const auto shifted = model.stream_shift(5);
    CHECK(shifted->info.tower_depth == model.info.tower_depth && shifted->info.param_count == model.info.param_count);
    CHECK(shifted->range_sites() == sites);
    CHECK(shifted->stream_shift(-5)->info.policy_len == model.info.policy_len);
    threw = false;
    try {
        model.stream_shift(25);
    } catch (const std::runtime_error &e) {
        threw = std::string(e.what()).find("[-24, 24]") != std::string::npos;
    }
    CHECK(threw);
    if (failures) return 1;
    printf("hip stream shift tests ok\n");
    return 0;
}
