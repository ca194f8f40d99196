// bench_symmetry_average.cpp — measurement, not a test: one executor thread evaluating Ataxx positions under all eight
// symmetries, averaged, two ways on the same model and boards, in interleaved rounds:
//   device   HipNetwork::set_average_symmetries          (kz_engine_submit_packed_decoded_avg: the engine fans out and averages)
//   host     AverageSymmetryNetwork<AtaxxSymBoard, HipNetwork>   (this thread maps, regenerates, searches, sums)
// Both through the blocking Network::evaluate_batch — the only call the wrapper has — with max_batch / 8 positions per call.
// Prints positions/s (= network evaluations / 8) and the thread's CPU share that is work: thread CPU time minus the time
// the HIP runtime spends polling inside kz_engine_wait*, over wall time.
//   bench_symmetry_average <ataxx-7 model.kzm> [seconds per round = 1] [rounds = 5] [max_batch = 256] [f16|f32]
// DESIGN.md §6.4.2 records what it printed.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <random>

#include "../../kzero_amd/csrc/host/hip_network.hpp"
#include "../../kzero_amd/csrc/host/symmetry.hpp"

using namespace kz::host;
using Net = HipNetwork<AtaxxSymBoard, AtaxxStdMapper>;

static std::vector<AtaxxSymBoard> random_boards(std::mt19937_64 &rng, const AtaxxStdMapper &m, size_t n) {
    std::vector<AtaxxSymBoard> boards(n);
    std::vector<size_t> indices(m.policy_len());
    std::iota(indices.begin(), indices.end(), (size_t)0);
    for (AtaxxSymBoard &b : boards) {
        b.size = m.size;
        for (int i = 0; i < m.size * m.size; i++) {
            const int r = (int)(rng() % 4);
            if (r == 0) b.tiles_next |= 1ull << i;
            if (r == 1) b.tiles_other |= 1ull << i;
        }
        std::shuffle(indices.begin(), indices.end(), rng);
        const size_t want = 1 + rng() % 60;
        std::vector<AtaxxMove> moves;
        for (size_t k = 0; k < indices.size() && moves.size() < want; k++)
            if (auto mv = m.index_to_move(indices[k])) moves.push_back(*mv);
        b.moves = moves;
    }
    return boards;
}

struct Round {
    double positions_per_s, work_share;
};

template <class N>
static Round run(N &net, Net &engine_side, const std::vector<AtaxxSymBoard> &boards, double seconds) {
    using clock = std::chrono::steady_clock;
    const auto t0 = clock::now();
    const uint64_t cpu0 = thread_cpu_ns(), wait0 = engine_side.wait_cpu_ns;
    size_t done = 0;
    double wall = 0;
    do {
        for (int i = 0; i < 16; i++) done += net.evaluate_batch(boards.data(), boards.size()).size();
        wall = std::chrono::duration<double>(clock::now() - t0).count();
    } while (wall < seconds);
    const double cpu = (double)(thread_cpu_ns() - cpu0) * 1e-9, wait = (double)(engine_side.wait_cpu_ns - wait0) * 1e-9;
    return {(double)done / wall, (cpu - wait) / wall};
}

int main(int argc, char **argv) {
    if (argc < 2) {
        std::fprintf(stderr, "usage: %s <ataxx-7 model.kzm> [seconds per round] [rounds] [max_batch] [f16|f32]\n", argv[0]);
        return 2;
    }
    const double seconds = argc > 2 ? atof(argv[2]) : 1.0;
    const int rounds = argc > 3 ? atoi(argv[3]) : 5;
    const size_t max_batch = argc > 4 ? (size_t)atoi(argv[4]) : 256;
    const int dtype = argc > 5 && !strcmp(argv[5], "f32") ? KZ_DTYPE_F32 : KZ_DTYPE_F16;
    const AtaxxStdMapper mapper(7);
    auto model = std::make_shared<const HipModel>(argv[1]);
    Net device(mapper, model, max_batch, 0, dtype);
    device.set_average_symmetries(d4_tables(mapper));
    Net inner(mapper, model, max_batch, 0, dtype);
    inner.set_device_decode(true);
    AverageSymmetryNetwork<AtaxxSymBoard, Net> host(std::move(inner));
    std::mt19937_64 rng(3);
    const auto boards = random_boards(rng, mapper, max_batch / 8);
    run(device, device, boards, 0.3);  // warm-up
    run(host, host.inner(), boards, 0.3);
    std::printf("{\"positions_per_call\": %zu, \"max_batch\": %zu, \"dtype\": \"%s\", \"rounds\": [", boards.size(), max_batch,
                dtype == KZ_DTYPE_F32 ? "f32" : "f16");
    for (int r = 0; r < rounds; r++) {
        const Round d = run(device, device, boards, seconds), h = run(host, host.inner(), boards, seconds);
        std::printf("%s\n {\"device_positions_per_s\": %.0f, \"device_thread_work_share\": %.3f, \"host_positions_per_s\": %.0f, "
                    "\"host_thread_work_share\": %.3f}", r ? "," : "", d.positions_per_s, d.work_share, h.positions_per_s, h.work_share);
    }
    std::printf("\n]}\n");
    return 0;
}
