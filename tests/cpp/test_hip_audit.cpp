// test_hip_audit.cpp — GPU test: the shadow audit through the C++ mirror (HipNetwork::set_audit / audit_stats ->
// kz_engine_set_audit / kz_engine_audit_stats).
//     test_hip_audit <an Ataxx 7x7 network, .kzm>
// Two f16 HipNetworks of 32 on the same model, one audited against exact f32 (period 1, 8 boards), one not; two evaluate_batch
// calls of 21 boards each.  The audit has compared 16 boards, and every evaluation equals the un-audited network's.
// Built against libkzhip.so and run by tests/test_hip_audit.py (-m gpu).
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
        std::fprintf(stderr, "usage: test_hip_audit <an Ataxx 7x7 network, .kzm>\n");
        return 2;
    }
    using Net = HipNetwork<AtaxxSymBoard, AtaxxStdMapper>;
    const AtaxxStdMapper mapper(7);
    auto model = std::make_shared<const HipModel>(argv[1]);
    std::mt19937_64 rng(3);
    const size_t n = 21;
    const auto first = random_boards(rng, mapper, n, 3), second = random_boards(rng, mapper, n, 5);

    Net plain(mapper, model, 32, 0, KZ_DTYPE_F16);
    plain.set_device_decode(true);
    Net audited(mapper, model, 32, 0, KZ_DTYPE_F16);
    audited.set_device_decode(true);

    // off: there is nothing to read
    bool threw = false;
    try {
        audited.audit_stats();
    } catch (const std::runtime_error &) {
        threw = true;
    }
    CHECK(threw);

    audited.set_audit(KZ_DTYPE_F32, 1, 8);
    for (const auto *boards : {&first, &second}) {
        const auto ref = plain.evaluate_batch(boards->data(), n);
        const auto out = audited.evaluate_batch(boards->data(), n);
        CHECK(ref.size() == n && out.size() == n);
        for (size_t i = 0; i < n && ref.size() == n && out.size() == n; i++) CHECK(same(out[i], ref[i]));
    }
    kz_audit_stats st = audited.audit_stats(true);
    CHECK(st.batches == 2 && st.boards == 16 && st.skipped == 0);
    CHECK(st.boards > 0 && st.moves > 0);
    CHECK(st.max_abs_prob > 0.0f);  // (f16 against exact f32: they differ somewhere)
    st = audited.audit_stats();
    CHECK(st.batches == 0 && st.boards == 0 && st.max_abs_prob == 0.0f);  // reset
    // the engine's own dtype is refused, and off is off
    threw = false;
    try {
        audited.set_audit(KZ_DTYPE_F16);
    } catch (const std::runtime_error &) {
        threw = true;
    }
    CHECK(threw);
    audited.set_audit(-1);
    const auto after = audited.evaluate_batch(first.data(), n), ref = plain.evaluate_batch(first.data(), n);
    for (size_t i = 0; i < n && after.size() == n && ref.size() == n; i++) CHECK(same(after[i], ref[i]));

    if (g_failed) {
        std::fprintf(stderr, "%d check(s) failed\n", g_failed);
        return 1;
    }
    std::puts("hip audit tests ok");
    return 0;
}
