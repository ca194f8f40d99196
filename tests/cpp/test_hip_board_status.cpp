// test_hip_board_status.cpp — GPU test: HipNetwork::evaluate_batch through the status entry (kz_engine_wait_decoded_status) and
// the exact-f32 range fallback (HipNetwork::set_range_fallback -> kz_engine_set_range_fallback).
//     test_hip_board_status <an Ataxx 7x7 network, .kzm>
// 37 boards in an f16 engine of 64; boards 0, 5 and 36 carry a scalar plane of 3e5 (moves_since_last_copy far beyond any game):
// finite in f32, inf as f16.  With the fallback on, evaluate_batch returns 37 evaluations, the three boards' are finite and equal
// to an exact-f32 HipNetwork's, the others equal to the same engine's on the batch without the cause, and the counter reads 3.
// With it off the call throws, naming the three boards.
// Built against libkzhip.so and run by tests/test_hip_board_status.py (-m gpu).
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

static bool same(const ZeroEvaluation &a, const ZeroEvaluation &b) {
    return a.values.value == b.values.value && a.values.wdl.win == b.values.wdl.win && a.values.wdl.draw == b.values.wdl.draw &&
           a.values.wdl.loss == b.values.wdl.loss && a.values.moves_left == b.values.moves_left && a.policy == b.policy;
}

int main(int argc, char **argv) {
    if (argc < 2) {
        std::fprintf(stderr, "usage: test_hip_board_status <an Ataxx 7x7 network, .kzm>\n");
        return 2;
    }
    using Net = HipNetwork<AtaxxSymBoard, AtaxxStdMapper>;
    const AtaxxStdMapper mapper(7);
    auto model = std::make_shared<const HipModel>(argv[1]);
    std::mt19937_64 rng(3);
    const size_t n = 37, range[3] = {0, 5, 36};
    const auto clean = random_boards(rng, mapper, n, 11);
    auto bad = clean;
    for (size_t b : range) bad[b].moves_since_last_copy = (int)(3e5f * (float)ATAXX_MAX_MOVES_SINCE_LAST_COPY);
    std::vector<float> scalars;
    BitBuffer buffer(input_bool_len(mapper));
    mapper.encode_input(buffer, scalars, bad[0]);
    CHECK(scalars[0] == 3e5f);

    Net net(mapper, model, 64, 0, KZ_DTYPE_F16);
    net.set_device_decode(true);
    const auto ref = net.evaluate_batch(clean.data(), n);
    CHECK(ref.size() == n && net.fell_back_boards == 0);

    // fallback off (the default): the batch fails, and the message names the three boards
    bool threw = false;
    try {
        net.evaluate_batch(bad.data(), n);
    } catch (const std::runtime_error &e) {
        threw = std::string(e.what()).find("non-finite activation") != std::string::npos &&
                std::string(e.what()).find("boards 0, 5, 36 ") != std::string::npos;
        if (!threw) std::fprintf(stderr, "unexpected message: %s\n", e.what());
    }
    CHECK(threw);

    // fallback on: 37 evaluations, three of them the exact-f32 engine's
    net.set_range_fallback(true);
    const auto out = net.evaluate_batch(bad.data(), n);
    CHECK(out.size() == n);
    CHECK(net.fell_back_boards == 3);
    Net exact(mapper, model, 64, 0, KZ_DTYPE_F32);
    exact.set_device_decode(true);
    std::vector<AtaxxSymBoard> three;
    for (size_t b : range) three.push_back(bad[b]);
    const auto ref32 = exact.evaluate_batch(three.data(), three.size());
    for (size_t i = 0, k = 0; i < out.size() && ref.size() == n && ref32.size() == 3; i++) {
        if (k < 3 && i == range[k]) {
            CHECK(std::isfinite(out[i].values.value) && std::isfinite(out[i].values.moves_left));
            CHECK(same(out[i], ref32[k]));
            k++;
        } else {
            CHECK(same(out[i], ref[i]));
        }
    }
    // the asynchronous pair counts too; a clean batch adds nothing
    auto again = bad;
    net.submit_batch(again.data(), n);
    CHECK(net.wait_batch().size() == n && net.fell_back_boards == 6);
    CHECK(net.evaluate_batch(clean.data(), n).size() == n && net.fell_back_boards == 6);
    // off again: it throws again
    net.set_range_fallback(false);
    threw = false;
    try {
        net.evaluate_batch(bad.data(), n);
    } catch (const std::runtime_error &) {
        threw = true;
    }
    CHECK(threw);
    // an exact-f32 engine has nothing to fall back from
    threw = false;
    try {
        exact.set_range_fallback(true);
    } catch (const std::runtime_error &) {
        threw = true;
    }
    CHECK(threw);

    if (g_failed) {
        std::fprintf(stderr, "%d check(s) failed\n", g_failed);
        return 1;
    }
    std::puts("hip board status tests ok");
    return 0;
}
