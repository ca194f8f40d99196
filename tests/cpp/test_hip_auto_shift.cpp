// test_hip_auto_shift.cpp — the shim chooses the stream shift: PositionSample (kzero_amd/csrc/host/position_sample.hpp),
// HipNetwork::set_position_sample, HipModel::range_profile_fast / auto_stream_shift, the KZ_HIP_STREAM_SHIFT parser.
//     test_hip_auto_shift --cpu                               the sample, the parser: no GPU
//     test_hip_auto_shift <an Ataxx 7x7 2x128 network, .kzm>  all of it
// A is the network of the file, B = A.stream_shift(-18): the same function on a stream 2^18 times as large.  An f16 HipNetwork of
// A with a sample (capacity 16, period 1, take 8) evaluates three batches of 21 boards; the sample then holds the first eight
// boards of the second and of the third batch, byte for byte.  B's profile on them has every board past 65504;
// B.auto_stream_shift returns k = shift_for(max board_max, 2); an f16 HipNetwork of the shifted model returns status 0 on every
// board and agrees with A's exact-f32 network within the decoded f16 contract of tests/test_gpu_parity.py (|dvalue, dwdl| <= 5e-3,
// |dprob| <= 2e-3; moves_left, a raw output: 3.5e-3 of max(1, |ref|)); B unshifted flags every board.
// Built against libkzhip.so and run by tests/test_hip_auto_shift.py.
#include <cstdio>
#include <cstring>
#include <numeric>
#include <random>
#include <set>
#include <thread>

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
        std::shuffle(indices.begin(), indices.end(), rng);
        const size_t want = 1 + rng() % 60;
        std::vector<AtaxxMove> moves;  // distinct moves in arbitrary order
        for (size_t k = 0; k < indices.size() && moves.size() < want; k++)
            if (auto mv = m.index_to_move(indices[k])) moves.push_back(*mv);
        b.moves = moves;
    }
    return boards;
}

static bool threw(const std::function<void()> &f) {
    try {
        f();
    } catch (const std::exception &) {
        return true;
    }
    return false;
}

// ---- no GPU: the ring, the prefix rule, two threads, the parser ----
static void cpu_tests() {
    {  // the first `take` boards of every `period`-th call; the oldest make room; snapshot oldest first
        PositionSample s(5, 2, 2);
        CHECK(threw([&] { const uint8_t b = 0; s.offer(&b, 1, nullptr, 1); }));  // no shape yet
        s.bind(3, 1);
        CHECK(s.size() == 0 && s.snapshot().boards == 0 && s.snapshot().bits.empty());
        uint8_t bits[4 * 4];  // four boards, stride 4 (one byte of padding each)
        float scalars[4];
        auto fill = [&](int call) {
            for (int b = 0; b < 4; b++) {
                for (int i = 0; i < 4; i++) bits[b * 4 + i] = i < 3 ? (uint8_t)(16 * call + 4 * b + i) : 0xff;
                scalars[b] = 100.0f * call + b;
            }
        };
        for (int call = 0; call < 7; call++) {  // calls 0, 2, 4, 6 are taken: boards (call, 0) and (call, 1)
            fill(call);
            s.offer(bits, 4, scalars, call == 4 ? 1 : 4);  // (call 4 has one board only)
        }
        const auto snap = s.snapshot();  // seven boards taken, the last five kept: (2,0) (2,1) (4,0) (6,0) (6,1)
        const int want[5][2] = {{2, 0}, {2, 1}, {4, 0}, {6, 0}, {6, 1}};
        CHECK(snap.boards == 5 && snap.bits_bytes == 3 && snap.n_scalar == 1 && snap.bits.size() == 15 && snap.scalars.size() == 5);
        for (int i = 0; i < 5 && snap.boards == 5; i++) {
            for (int j = 0; j < 3; j++) CHECK(snap.bits[i * 3 + j] == (uint8_t)(16 * want[i][0] + 4 * want[i][1] + j));
            CHECK(snap.scalars[i] == 100.0f * want[i][0] + want[i][1]);
        }
        s.bind(3, 1);  // the same shape again: nothing happens
        CHECK(s.size() == 5);
        s.bind(2, 0);  // another game: emptied
        CHECK(s.size() == 0);
        CHECK(threw([] { PositionSample bad(0); }));
    }
    {  // two threads: nothing lost, nothing twice
        const size_t calls = 2000, take = 3;
        PositionSample s(2 * calls * take, 1, take);
        s.bind(4, 1);
        auto worker = [&](uint32_t id) {
            for (uint32_t c = 0; c < calls; c++) {
                uint32_t words[5];
                float sc[5];
                for (uint32_t b = 0; b < 5; b++) {
                    words[b] = (id << 24) | (c << 4) | b;
                    sc[b] = (float)(c * 8 + b) + (id ? 0.5f : 0.0f);
                }
                s.offer(reinterpret_cast<const uint8_t *>(words), 4, sc, 5);
            }
        };
        std::thread a(worker, 0u), b(worker, 1u);
        a.join();
        b.join();
        const auto snap = s.snapshot();
        CHECK(snap.boards == 2 * calls * take);
        std::set<uint32_t> seen;
        bool consistent = true;
        for (size_t i = 0; i < snap.boards; i++) {
            uint32_t w;
            std::memcpy(&w, snap.bits.data() + 4 * i, 4);
            seen.insert(w);
            const uint32_t id = w >> 24, c = (w >> 4) & 0xfffff, bd = w & 15;
            consistent = consistent && bd < take && c < calls && snap.scalars[i] == (float)(c * 8 + bd) + (id ? 0.5f : 0.0f);
        }
        CHECK(seen.size() == snap.boards && consistent);  // every (thread, call, board < take) once, with its own scalars
    }
    {  // KZ_HIP_STREAM_SHIFT as hip.rs reads it
        CHECK(!StreamShiftEnv::parse(nullptr).automatic && StreamShiftEnv::parse(nullptr).k == 0);
        CHECK(StreamShiftEnv::parse("7").k == 7 && !StreamShiftEnv::parse("7").automatic && StreamShiftEnv::parse("-3").k == -3);
        CHECK(StreamShiftEnv::parse("auto").automatic && StreamShiftEnv::parse("auto").headroom_bits == 2);
        CHECK(StreamShiftEnv::parse("auto:4").automatic && StreamShiftEnv::parse("auto:4").headroom_bits == 4);
        for (const char *bad : {"", "auto:", "auto:x", "automatic", "3k", "k"}) CHECK(threw([&] { StreamShiftEnv::parse(bad); }));
    }
}

using Net = HipNetwork<AtaxxSymBoard, AtaxxStdMapper>;

// a board as HipNetwork packs it
static void pack(const AtaxxStdMapper &mapper, const AtaxxSymBoard &board, std::vector<uint8_t> &bits, std::vector<float> &scalars) {
    const size_t bool_count = input_bool_len(mapper), bits_bytes = (bool_count + 7) / 8;
    BitBuffer buffer(bool_count);
    mapper.encode_input(buffer, scalars, board);
    bits.insert(bits.end(), buffer.storage().begin(), buffer.storage().begin() + bits_bytes);
}

static void gpu_tests(const char *path) {
    const AtaxxStdMapper mapper(7);
    const int K = 18;
    auto A = std::make_shared<const HipModel>(path);
    std::shared_ptr<const HipModel> B = A->stream_shift(-K);
    CHECK(A->range_profile_fast_path() == "tower_resident_f32" && B->range_profile_fast_path() == "tower_resident_f32");
    std::mt19937_64 rng(3);
    const size_t n = 21;
    const std::vector<AtaxxSymBoard> batches[3] = {random_boards(rng, mapper, n), random_boards(rng, mapper, n), random_boards(rng, mapper, n)};

    // an empty sample: nothing measured, k = 0, the model itself
    auto sample = std::make_shared<PositionSample>(16, 1, 8);
    {
        const auto none = B->auto_stream_shift(0, *sample);
        CHECK(none.k == 0 && none.boards == 0 && none.max_abs == 0.0f && none.model.get() == B.get());
    }

    // A in f16 feeds the sample: evaluate_batch twice, the asynchronous pair once
    {
        Net a16(mapper, A, 32, 0, KZ_DTYPE_F16);
        a16.set_device_decode(true);
        a16.set_position_sample(sample);
        CHECK(a16.evaluate_batch(batches[0].data(), n).size() == n);
        CHECK(sample->size() == 8);
        CHECK(a16.evaluate_batch(batches[1].data(), n).size() == n);
        std::vector<AtaxxSymBoard> moved = batches[2];
        a16.submit_batch(moved.data(), n);
        CHECK(a16.wait_batch().size() == n);
    }
    std::vector<uint8_t> want_bits;
    std::vector<float> want_scalars;
    for (int batch = 1; batch < 3; batch++)
        for (size_t b = 0; b < 8; b++) pack(mapper, batches[batch][b], want_bits, want_scalars);
    const PositionSample::Snapshot snap = sample->snapshot();
    CHECK(snap.boards == 16 && snap.bits_bytes == (size_t)A->info.bits_bytes && snap.n_scalar == (size_t)A->info.input_scalar_channels);
    CHECK(snap.bits == want_bits && snap.scalars == want_scalars);

    // B's profile on those 16 boards: every board past 65504, and exactly 2^K times A's
    const auto pa = A->range_profile_fast(0, snap.bits.data(), snap.bits_bytes, snap.scalars.data(), (int)snap.boards);
    const auto pb = B->range_profile_fast(0, snap.bits.data(), snap.bits_bytes, snap.scalars.data(), (int)snap.boards);
    CHECK(pa.board_max.size() == 16 && pb.board_max.size() == 16);
    float m = 0.0f, lo = INFINITY;
    for (size_t b = 0; b < pb.board_max.size(); b++) {
        CHECK(pb.board_max[b] > 65504.0f && pb.board_max[b] == std::ldexp(pa.board_max[b], K));
        m = std::max(m, pb.board_max[b]);
        lo = std::min(lo, pb.board_max[b]);
    }
    CHECK(pb.site_max.back() == pa.site_max.back());  // (behind the final BN: the same tensor)
    const auto chosen = B->auto_stream_shift(0, *sample);
    std::printf("[auto shift] B = A << %d: board maxima %.0f .. %.0f on %zu boards -> k = %d\n", K, lo, m, chosen.boards, chosen.k);
    CHECK(chosen.boards == 16 && chosen.max_abs == m && chosen.k == shift_for(m, 2) && chosen.k >= 3);
    CHECK(chosen.model && chosen.model.get() != B.get());
    CHECK(B->auto_stream_shift(0, *sample, 0).k == shift_for(m, 0) && shift_for(m, 0) == chosen.k - 2);
    CHECK(A->auto_stream_shift(0, *sample).k == 0 && A->auto_stream_shift(0, *sample).model.get() == A.get());  // A needs none

    // the shifted model in f16: status 0 on every board (no throw, no fallback), the same function as A in exact f32
    Net a32(mapper, A, 32, 0, KZ_DTYPE_F32), s16(mapper, chosen.model, 32, 0, KZ_DTYPE_F16);
    a32.set_device_decode(true);
    s16.set_device_decode(true);
    float worst_v = 0.0f, worst_p = 0.0f, worst_ml = 0.0f;
    for (const auto &boards : batches) {
        const auto ref = a32.evaluate_batch(boards.data(), n);
        std::vector<ZeroEvaluation> out;
        CHECK(!threw([&] { out = s16.evaluate_batch(boards.data(), n); }));
        CHECK(out.size() == n && ref.size() == n);
        for (size_t i = 0; i < n && out.size() == n && ref.size() == n; i++) {
            const auto &o = out[i].values, &r = ref[i].values;
            worst_v = std::max({worst_v, std::fabs(o.value - r.value), std::fabs(o.wdl.win - r.wdl.win), std::fabs(o.wdl.draw - r.wdl.draw),
                                std::fabs(o.wdl.loss - r.wdl.loss)});
            worst_ml = std::max(worst_ml, std::fabs(o.moves_left - r.moves_left) / std::max(1.0f, std::fabs(r.moves_left)));
            CHECK(out[i].policy.size() == ref[i].policy.size());
            for (size_t j = 0; j < out[i].policy.size() && j < ref[i].policy.size(); j++)
                worst_p = std::max(worst_p, std::fabs(out[i].policy[j] - ref[i].policy[j]));
        }
    }
    std::printf("[auto shift] shifted f16 against A in exact f32: max |dvalue, dwdl| %.3e, max |dprob| %.3e, moves_left rel %.3e\n", worst_v,
                worst_p, worst_ml);
    CHECK(s16.fell_back_boards == 0);
    CHECK(worst_v <= 5e-3f && worst_p <= 2e-3f && worst_ml <= 3.5e-3f);

    // B unshifted in f16: every board out of range
    {
        kz_engine *raw = nullptr;
        kz_check(kz_engine_create(B->get(), 0, 16, KZ_DTYPE_F16, &raw));
        std::vector<int64_t> offsets(17, 0);  // no moves: the range check alone speaks
        std::vector<float> values(16 * 5), probs(1);
        std::vector<uint8_t> status(16, 0);
        const int32_t no_move = 0;
        const int rc = kz_engine_eval_packed_decoded_status(raw, snap.bits.data(), snap.bits_bytes, snap.scalars.data(), 16, nullptr, offsets.data(),
                                                            &no_move, values.data(), probs.data(), status.data());
        CHECK(rc == 0);
        for (size_t b = 0; b < 16; b++) CHECK(status[b] & KZ_BOARD_NONFINITE);
        kz_engine_destroy(raw);
    }

    // a stream that is not finite in f32 is not a shift's business: the call throws and names the board count
    {
        auto bad = std::make_shared<PositionSample>(4, 1, 4);
        bad->bind(snap.bits_bytes, snap.n_scalar);
        std::vector<float> sc(snap.scalars.begin(), snap.scalars.begin() + 3 * snap.n_scalar);
        sc[snap.n_scalar] = INFINITY;
        bad->offer(snap.bits.data(), snap.bits_bytes, sc.data(), 3);
        std::string what;
        try {
            B->auto_stream_shift(0, *bad);
        } catch (const std::runtime_error &e) {
            what = e.what();
        }
        CHECK(what.find("not finite") != std::string::npos && what.find("3 sampled boards") != std::string::npos);
    }
}

int main(int argc, char **argv) {
    if (argc < 2) {
        std::fprintf(stderr, "usage: test_hip_auto_shift --cpu | <an Ataxx 7x7 2x128 network, .kzm>\n");
        return 2;
    }
    cpu_tests();
    if (std::string(argv[1]) != "--cpu") gpu_tests(argv[1]);
    if (g_failed) {
        std::fprintf(stderr, "%d check(s) failed\n", g_failed);
        return 1;
    }
    std::puts("hip auto shift tests ok");
    return 0;
}
