// test_hip_symmetry_average.cpp — GPU test: HipNetwork::set_average_symmetries (every board under every symmetry averaged
// inside the engine: kz_engine_submit_packed_decoded_avg) against AverageSymmetryNetwork<AtaxxSymBoard, HipNetwork> (the host
// wrapper: boards mapped eight times, move lists regenerated and searched, the replies summed on this thread), on the golden
// Ataxx network.   test_hip_symmetry_average <tests/golden/ataxx7_2x16.kzm>
//
// VALUES must be equal.  Both routes put the same 8 n planes through the same launch (the wrapper's 64 / 24 mapped boards are
// one batch of the inner engine of 64, in the order of the device's virtual batch) and both then compute
// (((0 + v_0) + v_1) + ... + v_7) / 8 in f32 — average_evals (host/symmetry.hpp) folds in k order and divides once, as
// symmetry.rs:156-160 does and as include/kz_hip.h states for the device.
//
// PROBABILITIES.  Both routes compute ((0 + p_0 / 8) + p_1 / 8) + ... in k order (average_evals adds `policy / n` per symmetry
// in ascending k: the reference's order, symmetry.rs:166-176, so nothing is added for the wrapper's order).  What differs is
// p_k itself: the wrapper's mapped move list is sorted by policy index, so its per-symmetry softmax sums the same n
// exponentials in another order than the device, which sums in the board's own move order.  As test_hip_symmetry.cpp
// derives, two sums of n positive f32 terms differ by at most 2 (n - 1) u relative (u = 2^-24) and each quotient rounds once
// more:  |p_k - p_k'| <= 2 n u p_k  with n the board's move count.  The eight-term average adds its own roundings on either
// side: one per quotient p_k / 8 and one per addition, every partial sum of positive terms being at most the final one —
// (8 + 1) u relative for each route to first order.  With A the wrapper's average:
//     |A - A'| <= (2 n + 2 (8 + 1)) u' A,      u' = 1.01 * 2^-24 (the second-order terms of at most 2 n + 18 <= 140 roundings).
// Built against libkzhip.so and run by tests/test_symmetry_average.py (-m gpu).
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

static std::vector<AtaxxSymBoard> random_boards(std::mt19937_64 &rng, const AtaxxStdMapper &m, size_t n, size_t finished) {
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
        if (bi == finished) continue;  // a finished game: no moves
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
    if (host.size() != boards.size() || device.size() != boards.size()) return;
    const double u = 1.01 * std::ldexp(1.0, -24);
    double worst = 0;
    for (size_t i = 0; i < boards.size(); i++) {
        const ZeroValuesPov &a = host[i].values, &b = device[i].values;
        CHECK(a.value == b.value && a.wdl.win == b.wdl.win && a.wdl.draw == b.wdl.draw && a.wdl.loss == b.wdl.loss && a.moves_left == b.moves_left);
        const size_t n = boards[i].moves ? boards[i].moves->size() : 0;
        CHECK(host[i].policy.size() == n && device[i].policy.size() == n);
        const double bound = (2.0 * (double)n + 2.0 * (8 + 1)) * u;
        for (size_t k = 0; k < n && k < device[i].policy.size() && k < host[i].policy.size(); k++) {
            const double p = host[i].policy[k], q = device[i].policy[k];
            CHECK(p > 0 && std::fabs(p - q) <= bound * p);
            worst = std::max(worst, std::fabs(p - q) / p / bound);
        }
    }
    std::printf("worst |dp| / p = %.3f of the bound\n", worst);
}

int main(int argc, char **argv) {
    if (argc < 2) {
        std::fprintf(stderr, "usage: test_hip_symmetry_average <tests/golden/ataxx7_2x16.kzm>\n");
        return 2;
    }
    using Net = HipNetwork<AtaxxSymBoard, AtaxxStdMapper>;
    const AtaxxStdMapper mapper(7);
    auto model = std::make_shared<const HipModel>(argv[1]);
    std::mt19937_64 rng(3);
    for (int dtype : {KZ_DTYPE_F16, KZ_DTYPE_F32}) {
        Net inner(mapper, model, 64, 0, dtype);
        inner.set_device_decode(true);
        AverageSymmetryNetwork<AtaxxSymBoard, Net> host(std::move(inner));
        Net device(mapper, model, 64, 0, dtype);
        device.set_average_symmetries(d4_tables(mapper));
        CHECK(device.max_batch_size() == 64);  // (keeps its meaning: the engine's)

        // 8 boards = max_batch / n_sym, one of them finished; then a ragged 3
        const auto eight = random_boards(rng, mapper, 8, 5);
        const auto dev8 = device.evaluate_batch(eight.data(), eight.size());
        compare(eight, host.evaluate_batch(eight.data(), eight.size()), dev8);
        CHECK(dev8.size() == 8 && dev8[5].policy.empty());
        const auto three = random_boards(rng, mapper, 3, 99);
        compare(three, host.evaluate_batch(three.data(), three.size()), device.evaluate_batch(three.data(), three.size()));

        // more boards than max_batch / n_sym: evaluate_batch goes through the engine in chunks of 8 — the same calls as 8 + 8 + 3
        const auto many = random_boards(rng, mapper, 19, 7);
        const auto all19 = device.evaluate_batch(many.data(), many.size());
        CHECK(all19.size() == 19);
        for (size_t lo = 0; lo < 19 && all19.size() == 19; lo += 8) {
            const auto part = device.evaluate_batch(many.data() + lo, std::min<size_t>(8, 19 - lo));
            for (size_t i = 0; i < part.size(); i++)
                CHECK(part[i].values.value == all19[lo + i].values.value && part[i].policy == all19[lo + i].policy);
        }

        // the asynchronous pair: two averaged batches in flight, results in submission order
        std::vector<AtaxxSymBoard> c8 = eight, c3 = three;  // (submit_batch moves the boards out)
        device.submit_batch(c8.data(), c8.size());
        device.submit_batch(c3.data(), c3.size());
        const auto again8 = device.wait_batch(), again3 = device.wait_batch();
        CHECK(again8.size() == dev8.size());
        for (size_t i = 0; i < again8.size() && i < dev8.size(); i++)
            CHECK(again8[i].values.value == dev8[i].values.value && again8[i].policy == dev8[i].policy);
        CHECK(again3.size() == 3);

        // the average is really over the symmetries: it differs from the plain evaluation
        Net plain(mapper, model, 64, 0, dtype);
        plain.set_device_decode(true);
        const auto p8 = plain.evaluate_batch(eight.data(), eight.size());
        size_t differ = 0;
        for (size_t i = 0; i < 8; i++) differ += p8[i].values.value != dev8[i].values.value;
        CHECK(differ >= 6);

        // one or the other
        bool threw = false;
        try {
            device.set_random_symmetries(d4_tables(mapper), std::mt19937_64(1));
        } catch (const std::logic_error &) {
            threw = true;
        }
        CHECK(threw);
    }
    if (g_failed) {
        std::fprintf(stderr, "%d check(s) failed\n", g_failed);
        return 1;
    }
    std::puts("hip symmetry average tests ok");
    return 0;
}
