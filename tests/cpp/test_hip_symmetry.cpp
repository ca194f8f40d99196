// test_hip_symmetry.cpp — GPU test: HipNetwork::set_random_symmetries (the symmetry inside the launch: ids and two tables
// handed to the engine) against RandomSymmetryNetwork<HipNetwork> (the host wrapper: boards mapped, move lists regenerated
// and searched on this thread) with the same id sequence, on an Ataxx network.   test_hip_symmetry <model.kzm>
// Values must be equal: both routes put the same planes through the same launch.  A move's probability differs by the order
// of the softmax sum only — the wrapper's mapped move list is sorted by policy index, the device sums in the board's own move
// order: two sums of n positive f32 terms differ by at most 2 (n - 1) 2^-24 relative, each quotient rounds once more:
// |dp| / p <= 2 n 2^-24 with n the board's move count.
// Built against libkzhip.so and run by tests/test_symmetry_tables.py (-m gpu).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <numeric>
#include <random>

#include "../../kzero_amd/csrc/host/hip_network.hpp"
#include "../../kzero_amd/csrc/host/symmetry.hpp"

using namespace kz::host;

static int g_failed = 0;
#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) {                                                           \
            std::fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            g_failed++;                                                          \
        }                                                                        \
    } while (0)

static std::vector<AtaxxSymBoard> random_boards(std::mt19937_64 &rng, const AtaxxStdMapper &m, size_t n) {
    std::vector<AtaxxSymBoard> boards(n);
    std::vector<size_t> indices(m.policy_len());
    std::iota(indices.begin(), indices.end(), (size_t)0);
    for (size_t bi = 0; bi < n; bi++) {
        AtaxxSymBoard &b = boards[bi];
        b.size = m.size;
        for (int i = 0; i < m.size * m.size; i++) {
            const int r = (int)(rng() % 4);
            if (r == 0) b.tiles_next |= 1ull << i;
            if (r == 1) b.tiles_other |= 1ull << i;
            if (r == 2 && rng() % 4 == 0) b.gaps |= 1ull << i;
        }
        b.moves_since_last_copy = (int)(rng() % 100);
        if (bi == 5) continue;  // a finished game: no moves
        std::shuffle(indices.begin(), indices.end(), rng);
        const size_t want = 1 + rng() % 60;
        std::vector<AtaxxMove> moves;  // distinct moves in arbitrary order
        for (size_t k = 0; k < indices.size() && moves.size() < want; k++)
            if (auto mv = m.index_to_move(indices[k])) moves.push_back(*mv);
        b.moves = moves;
    }
    return boards;
}

static void compare(const std::vector<AtaxxSymBoard> &boards, const std::vector<ZeroEvaluation> &host, const std::vector<ZeroEvaluation> &device) {
    CHECK(host.size() == boards.size() && device.size() == boards.size());
    double worst = 0;
    for (size_t i = 0; i < boards.size(); i++) {
        const ZeroValuesPov &a = host[i].values, &b = device[i].values;
        CHECK(a.value == b.value && a.wdl.win == b.wdl.win && a.wdl.draw == b.wdl.draw && a.wdl.loss == b.wdl.loss && a.moves_left == b.moves_left);
        const size_t n = boards[i].moves ? boards[i].moves->size() : 0;
        CHECK(host[i].policy.size() == n && device[i].policy.size() == n);
        const double bound = 2.0 * (double)n * std::ldexp(1.0, -24);
        for (size_t k = 0; k < n && k < device[i].policy.size() && k < host[i].policy.size(); k++) {
            const double p = host[i].policy[k], q = device[i].policy[k];
            CHECK(p > 0 && std::fabs(p - q) <= bound * p);
            worst = std::max(worst, std::fabs(p - q) / p / (bound > 0 ? bound : 1));
        }
    }
    std::printf("worst |dp| / p = %.3f of the bound\n", worst);
}

int main(int argc, char **argv) {
    if (argc < 2) {
        std::fprintf(stderr, "usage: test_hip_symmetry <ataxx-7 model.kzm>\n");
        return 2;
    }
    using Net = HipNetwork<AtaxxSymBoard, AtaxxStdMapper>;
    const AtaxxStdMapper mapper(7);
    auto model = std::make_shared<const HipModel>(argv[1]);
    const uint64_t seed = 9;

    Net inner(mapper, model, 64, 0, KZ_DTYPE_F16);
    inner.set_device_decode(true);
    RandomSymmetryNetwork<AtaxxSymBoard, Net> host(std::move(inner), std::mt19937_64(seed), true);
    Net device(mapper, model, 64, 0, KZ_DTYPE_F16);
    device.set_random_symmetries(d4_tables(mapper), std::mt19937_64(seed));

    std::mt19937_64 rng(3);
    // blocking calls, ragged batches: both draw one id per board, in board order, from equal generators
    for (size_t n : {(size_t)37, (size_t)64, (size_t)1}) {
        const auto boards = random_boards(rng, mapper, n);
        compare(boards, host.evaluate_batch(boards.data(), n), device.evaluate_batch(boards.data(), n));
    }
    // the asynchronous pair with three batches in flight: ids are drawn at submit, in submission order
    std::vector<std::vector<AtaxxSymBoard>> batches;
    for (size_t n : {(size_t)40, (size_t)23, (size_t)64}) batches.push_back(random_boards(rng, mapper, n));
    for (auto &b : batches) {
        std::vector<AtaxxSymBoard> copy = b;  // (submit_batch moves the boards out)
        device.submit_batch(copy.data(), copy.size());
    }
    for (auto &b : batches) compare(b, host.evaluate_batch(b.data(), b.size()), device.wait_batch());

    // the symmetry is really applied: with the identity alone the device route is the plain network
    {
        Net plain(mapper, model, 64, 0, KZ_DTYPE_F16);
        plain.set_device_decode(true);
        const auto boards = random_boards(rng, mapper, 37);
        const auto a = plain.evaluate_batch(boards.data(), boards.size());
        const auto b = device.evaluate_batch(boards.data(), boards.size());
        size_t differ = 0;
        for (size_t i = 0; i < boards.size(); i++) differ += a[i].values.value != b[i].values.value;
        CHECK(differ > boards.size() / 2);  // (ids 1..7 on about 7 boards of 8)
    }
    if (g_failed) {
        std::fprintf(stderr, "%d check(s) failed\n", g_failed);
        return 1;
    }
    std::puts("hip symmetry tests ok");
    return 0;
}
