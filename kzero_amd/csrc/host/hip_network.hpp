// hip_network.hpp — `HipNetwork<B, M>`: the executor behind the `Network` contract, C++ mirror of the Rust shim in
// kzero_amd/rust/hip.rs.  Same shape as `CudaNetwork` (rust/kz-core/src/network/cudnn.rs:18-88): encode every board
// with the mapper, run the engine, decode the outputs.  Talks to the product only through the C ABI.
#pragma once
#include <algorithm>
#include <atomic>
#include <cmath>
#include <condition_variable>
#include <cstdlib>
#include <exception>
#include <functional>
#include <iterator>
#include <memory>
#include <mutex>
#include <random>
#include <stdexcept>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>

#include <time.h>

#include "../../../include/kz_hip.h"
#include "mapping.hpp"
#include "network.hpp"
#include "position_sample.hpp"
#include "symmetry.hpp"

namespace kz::host {

// A board type may carry the policy indices of its available moves, computed where the board was made (a generator
// thread): `const std::vector<int32_t> *policy_indices() const`, null when it does not.  The executor thread then
// neither generates the moves nor looks them up for the device-side decode.
template <class T, class = void>
struct has_policy_indices : std::false_type {};
template <class T>
struct has_policy_indices<T, std::void_t<decltype(std::declval<const T &>().policy_indices())>> : std::true_type {};

// CPU time of the calling thread (measurement: how much of an executor thread's time is work, how much is the HIP
// runtime spinning in kz_engine_wait*)
inline uint64_t thread_cpu_ns() {
    timespec ts{};
    clock_gettime(CLOCK_THREAD_CPUTIME_ID, &ts);
    return (uint64_t)ts.tv_sec * 1000000000ull + (uint64_t)ts.tv_nsec;
}

inline void kz_check(int rc) {
    if (rc != 0) throw std::runtime_error(std::string("kzhip: ") + kz_last_error());  // the reference panics
}

// One persistent helper thread that runs a job handed over by its owner while the owner does its own share of the same
// work (HipNetwork::prepare: half of a batch's board encoding and move-list building each).  start() hands over, finish()
// waits and re-throws what the job threw.  Not part of the reference: its executor thread does all of a batch's host work
// alone (cudnn.rs:55-87), which at 500k evals/s per GPU is most of a core.
class PrepHelper {
    std::mutex m_;
    std::condition_variable cv_;
    std::function<void()> job_;
    bool busy_ = false, quit_ = false;
    std::exception_ptr err_;
    std::thread th_;

    void run() {
        std::unique_lock<std::mutex> l(m_);
        for (;;) {
            cv_.wait(l, [&] { return quit_ || job_; });
            if (quit_) return;
            std::function<void()> j = std::move(job_);
            job_ = nullptr;
            l.unlock();
            std::exception_ptr err;
            try {
                j();
            } catch (...) {
                err = std::current_exception();
            }
            cpu_ns = thread_cpu_ns();
            l.lock();
            err_ = err;
            busy_ = false;
            cv_.notify_all();
        }
    }

  public:
    std::atomic<uint64_t> cpu_ns{0};  // CPU time of the helper thread so far (measurement)
    PrepHelper() : th_([this] { run(); }) {}
    PrepHelper(const PrepHelper &) = delete;
    ~PrepHelper() {
        {
            std::lock_guard<std::mutex> l(m_);
            quit_ = true;
        }
        cv_.notify_all();
        th_.join();
    }
    void start(std::function<void()> job) {
        {
            std::lock_guard<std::mutex> l(m_);
            job_ = std::move(job);
            busy_ = true;
        }
        cv_.notify_all();
    }
    void finish() {
        std::unique_lock<std::mutex> l(m_);
        cv_.wait(l, [&] { return !busy_; });
        if (err_) {
            std::exception_ptr e = err_;
            err_ = nullptr;
            std::rethrow_exception(e);
        }
    }
};

// The k of HipModel::stream_shift for a stream whose shifted sites reach max_abs (include/kz_hip.h):
// k = max(0, ceil(log2(max_abs / 65504)) + headroom_bits), from frexp: no floating-point logarithm.  The library reports
// (range_profile) and applies (stream_shift); the caller decides.
inline int shift_for(float max_abs, int headroom_bits = 2) {
    if (!std::isfinite(max_abs) || max_abs < 0) throw std::invalid_argument("shift_for: max_abs must be finite and non-negative");
    if (max_abs == 0) return 0;
    int e = 0;
    const double mant = std::frexp((double)max_abs / 65504.0, &e);  // max_abs / 65504 = mant * 2^e, mant in [0.5, 1)
    const int ceil_log2 = mant == 0.5 ? e - 1 : e;
    return std::max(0, ceil_log2 + headroom_bits);
}

// What a stream shift of k does to the stored values a range histogram counted (HipModel::range_histogram: hist
// [n_sites][KZ_RANGE_BINS], include/kz_hip.h), per site: E' = E - k on the shifted sites, E' = E on the last one.
//   f16_over E' >= 16; f16_top E' = 15 (the binade of 65504 .. 65536); f16_subnormal -25 <= E' <= -15; f16_flushed E' < -25;
//   split_lo_subnormal E' <= -3 (the lo half of a split16 pair is subnormal or gone)
//   clamped_low, clamped_high: the two end bins (E <= -50, E >= 43) as they are — for every k in [-24, 24] they lie in
//   f16_flushed (and split_lo_subnormal) and in f16_over, so nothing is guessed
// Integer arithmetic only; the library reports, the caller decides.
struct ShiftReport {
    uint64_t total = 0, zero = 0, nonfinite = 0, f16_over = 0, f16_top = 0, f16_subnormal = 0, f16_flushed = 0,
             split_lo_subnormal = 0, clamped_low = 0, clamped_high = 0;
};
inline std::vector<ShiftReport> shift_report(const std::vector<uint64_t> &hist, int k) {
    if (hist.empty() || hist.size() % KZ_RANGE_BINS) throw std::invalid_argument("shift_report: hist must be [n_sites][96]");
    if (k < -24 || k > 24) throw std::invalid_argument("shift_report: k out of range [-24, 24]");
    const size_t n = hist.size() / KZ_RANGE_BINS;
    std::vector<ShiftReport> out(n);
    for (size_t site = 0; site < n; site++) {
        const uint64_t *row = hist.data() + site * KZ_RANGE_BINS;
        const int shift = site + 1 < n ? k : 0;
        ShiftReport &r = out[site];
        for (int b = 0; b < KZ_RANGE_BINS; b++) r.total += row[b];
        r.zero = row[0];
        r.nonfinite = row[KZ_RANGE_BINS - 1];
        r.clamped_low = row[1];
        r.clamped_high = row[KZ_RANGE_BINS - 2];
        for (int b = 1; b < KZ_RANGE_BINS - 1; b++) {
            const int e = b - 51 - shift;  // (bin 1: at most this; bin 94: at least this — the classes hold for both)
            if (e >= 16) r.f16_over += row[b];
            if (e == 15) r.f16_top += row[b];
            if (e >= -25 && e <= -15) r.f16_subnormal += row[b];
            if (e < -25) r.f16_flushed += row[b];
            if (e <= -3) r.split_lo_subnormal += row[b];
        }
    }
    return out;
}

// the `Arc<Graph>` of the reference: immutable, shared by every executor
// (auto_stream_shift hands the model itself back when no shift is needed: for that call it must live in a shared_ptr)
class HipModel : public std::enable_shared_from_this<HipModel> {
    kz_model *ptr_ = nullptr;

    explicit HipModel(kz_model *adopted) : ptr_(adopted) { kz_check(kz_model_get_info(ptr_, &info)); }

  public:
    kz_model_info info{};
    explicit HipModel(const std::string &path) {
        kz_check(kz_model_load(path.c_str(), &ptr_));
        kz_check(kz_model_get_info(ptr_, &info));
    }
    HipModel(const void *blob, size_t len) {
        kz_check(kz_model_load_memory(blob, len, &ptr_));
        kz_check(kz_model_get_info(ptr_, &info));
    }
    HipModel(const HipModel &) = delete;
    HipModel &operator=(const HipModel &) = delete;
    ~HipModel() { kz_model_free(ptr_); }
    const kz_model *get() const { return ptr_; }

    // The same function with a residual stream 2^-k times as large (kz_model_stream_shift): a new model, k in [-24, 24].
    std::shared_ptr<const HipModel> stream_shift(int k) const {
        kz_model *out = nullptr;
        kz_check(kz_model_stream_shift(ptr_, k, &out));
        return std::shared_ptr<const HipModel>(new HipModel(out));
    }
    // the names of the range profile's sites, in order
    std::vector<std::string> range_sites() const {
        int n = 0;
        kz_check(kz_model_range_sites(ptr_, &n));
        std::vector<std::string> names;
        for (int site = 0; site < n; site++) {
            char buf[32];
            kz_check(kz_model_range_site_name(ptr_, site, buf, sizeof buf));
            names.emplace_back(buf);
        }
        return names;
    }
    // max |x| of every stored tower tensor on `batch` packed boards, exact f32 on `device` (kz_model_range_profile):
    // site_max [n_sites] over all boards, board_max [batch] over the sites a shift moves
    struct RangeProfile {
        std::vector<float> site_max, board_max;
    };
    RangeProfile range_profile(int device, const uint8_t *bits, size_t bits_stride, const float *scalars_in, int batch) const {
        int n = 0;
        kz_check(kz_model_range_sites(ptr_, &n));
        RangeProfile r{std::vector<float>((size_t)n), std::vector<float>((size_t)std::max(batch, 0))};
        kz_check(kz_model_range_profile(ptr_, device, bits, bits_stride, scalars_in, batch, r.site_max.data(), r.board_max.data()));
        return r;
    }
    // The same profile at the rate of the one-launch exact-f32 tower where that kernel takes the network, and exactly
    // range_profile elsewhere (kz_model_range_profile_fast); range_profile_fast_path says which, without a GPU.
    RangeProfile range_profile_fast(int device, const uint8_t *bits, size_t bits_stride, const float *scalars_in, int batch) const {
        int n = 0;
        kz_check(kz_model_range_sites(ptr_, &n));
        RangeProfile r{std::vector<float>((size_t)n), std::vector<float>((size_t)std::max(batch, 0))};
        kz_check(kz_model_range_profile_fast(ptr_, device, bits, bits_stride, scalars_in, batch, r.site_max.data(), r.board_max.data()));
        return r;
    }
    // How many stored values of every site lie in each binade, counted in exact f32 on `device`: [n_sites][KZ_RANGE_BINS], every
    // site summing to batch * h * w * tower_channels (kz_model_range_histogram_fast: inside the one-launch tower where
    // range_profile_fast_path says so; fast = false: kz_model_range_histogram, per layer).  shift_report reads it.
    std::vector<uint64_t> range_histogram(int device, const uint8_t *bits, size_t bits_stride, const float *scalars_in, int batch,
                                          bool fast = true) const {
        int n = 0;
        kz_check(kz_model_range_sites(ptr_, &n));
        std::vector<uint64_t> hist((size_t)n * KZ_RANGE_BINS);
        kz_check((fast ? kz_model_range_histogram_fast : kz_model_range_histogram)(ptr_, device, bits, bits_stride, scalars_in, batch,
                                                                                  (void *)hist.data()));
        return hist;
    }
    std::string range_profile_fast_path() const {
        char buf[32];
        kz_check(kz_model_range_profile_fast_path(ptr_, buf, sizeof buf));
        return buf;
    }

    // The shift this network needs on the positions of `sample`: range_profile_fast on a snapshot, m = the largest board_max,
    // k = shift_for(m, headroom_bits); `model` is stream_shift(k), or this model itself for k == 0.  An empty sample gives
    // k = 0 and boards == 0 (the first network of a run: pair it with the range fallback).  m = +inf throws: a network that
    // overflows f32 is not a shift's business.
    struct AutoShift {
        std::shared_ptr<const HipModel> model;
        int k = 0;
        float max_abs = 0.0f;
        size_t boards = 0;     // boards profiled; 0: the sample was empty and nothing was measured
    };
    AutoShift auto_stream_shift(int device, const PositionSample &sample, int headroom_bits = 2) const {
        AutoShift r;
        const PositionSample::Snapshot snap = sample.snapshot();
        r.boards = snap.boards;
        if (snap.boards) {
            if (snap.bits_bytes != (size_t)info.bits_bytes || snap.n_scalar != (size_t)info.input_scalar_channels)
                throw std::invalid_argument("auto_stream_shift: the sample holds boards of another shape than this model's");
            const RangeProfile p = range_profile_fast(device, snap.bits.data(), snap.bits_bytes, snap.scalars.data(), (int)snap.boards);
            r.max_abs = *std::max_element(p.board_max.begin(), p.board_max.end());
            if (!std::isfinite(r.max_abs))
                throw std::runtime_error("kzhip: auto_stream_shift: the residual stream is not finite in exact f32 on the " +
                                         std::to_string(snap.boards) + " sampled boards: no shift brings such a network into range");
            r.k = shift_for(r.max_abs, headroom_bits);
        }
        r.model = r.k ? stream_shift(r.k) : shared_from_this();
        return r;
    }
};

// KZ_HIP_STREAM_SHIFT as the Rust shim reads it (hip.rs: StreamShift::from_env; read here, never by the library): unset or 0:
// the network as trained; <k>: stream_shift(k); auto[:<headroom>]: the k its own positions ask for (auto_stream_shift).
struct StreamShiftEnv {
    bool automatic = false;
    int k = 0, headroom_bits = 2;
    static StreamShiftEnv parse(const char *v) {
        StreamShiftEnv e;
        if (!v) return e;
        const std::string s(v);
        const auto number = [&](const std::string &t, int &out) {
            size_t used = 0;
            try {
                out = std::stoi(t, &used);
            } catch (const std::exception &) {
                used = 0;
            }
            if (t.empty() || used != t.size())
                throw std::invalid_argument("KZ_HIP_STREAM_SHIFT must be an integer in [-24, 24] or auto[:<headroom bits>], got '" + s + "'");
        };
        if (s == "auto") e.automatic = true;
        else if (s.rfind("auto:", 0) == 0) {
            e.automatic = true;
            number(s.substr(5), e.headroom_bits);
        } else number(s, e.k);
        return e;
    }
    static StreamShiftEnv from_env() { return parse(std::getenv("KZ_HIP_STREAM_SHIFT")); }
};

// the sample KZ_HIP_STREAM_SHIFT=auto profiles: process-wide, fed by every HipNetwork (the first 64 boards of every batch, the
// most recent 16384 kept: 2 MB for chess)
inline const std::shared_ptr<PositionSample> &process_position_sample() {
    static const std::shared_ptr<PositionSample> sample = std::make_shared<PositionSample>(16384, 1, 64);
    return sample;
}

// What the loader applies to every network it loads (server_hip.rs: load_graph).  The first network of a run, with no
// positions sampled yet, stays unshifted.
inline std::shared_ptr<const HipModel> stream_shift_from_env(std::shared_ptr<const HipModel> model, int device) {
    const StreamShiftEnv e = StreamShiftEnv::from_env();
    if (e.automatic) return model->auto_stream_shift(device, *process_position_sample(), e.headroom_bits).model;
    return e.k ? model->stream_shift(e.k) : model;
}

template <class B, class M>
class HipNetwork : public Network<B> {
    M mapper_;
    std::shared_ptr<const HipModel> model_;
    kz_engine *engine_ = nullptr;
    size_t max_batch_size_;
    std::vector<uint8_t> bits_;
    std::vector<float> scalars_in_;
    // asynchronous pair: the boards of every batch in flight (decode_output needs their legal moves), oldest first
    std::vector<B> pending_boards_[KZ_ENGINE_SLOTS];
    int next_slot_ = 0, oldest_slot_ = 0, in_flight_ = 0;
    // decode_output on the device (kz_engine_submit_packed_decoded / kz_engine_wait_decoded): the CSR move lists of
    // the batches in flight
    bool device_decode_ = false;
    std::vector<int64_t> move_offsets_[KZ_ENGINE_SLOTS];
    std::vector<int32_t> move_indices_;
    // random symmetries inside the launch (set_random_symmetries): one id per board, drawn at submit
    int n_sym_ = 0;
    std::mt19937_64 sym_rng_;
    std::vector<uint8_t> sym_ids_;
    // every board under all n_sym_ symmetries, averaged inside the engine (set_average_symmetries)
    bool average_ = false;
    // the boards just packed are offered to this sample (set_position_sample; null: off)
    std::shared_ptr<PositionSample> sample_;
    void offer_sample(size_t bits_bytes, size_t n) {
        if (sample_) sample_->offer(bits_.data(), bits_bytes, scalars_in_.data(), n);
    }

    // the decoded submit of a prepared batch; with symmetries on, every board gets an id of its own (symmetry.rs:47-52)
    void submit_decoded(int slot, size_t bits_bytes, size_t n) {
        if (average_) {
            kz_check(kz_engine_submit_packed_decoded_avg(engine_, slot, bits_.data(), bits_bytes, scalars_in_.data(), (int)n,
                                                         move_offsets_[slot].data(), move_indices_.data()));
            return;
        }
        if (!n_sym_) {
            kz_check(kz_engine_submit_packed_decoded(engine_, slot, bits_.data(), bits_bytes, scalars_in_.data(), (int)n,
                                                     move_offsets_[slot].data(), move_indices_.data()));
            return;
        }
        std::uniform_int_distribution<int> dist(0, n_sym_ - 1);
        sym_ids_.resize(n);
        for (size_t i = 0; i < n; i++) sym_ids_[i] = (uint8_t)dist(sym_rng_);
        kz_check(kz_engine_submit_packed_decoded_sym(engine_, slot, bits_.data(), bits_bytes, scalars_in_.data(), (int)n, sym_ids_.data(),
                                                     move_offsets_[slot].data(), move_indices_.data()));
    }

    // ---- a batch's host work before the launch: encode_input of every board (cudnn.rs:61-64) and, with the decode on the
    // device, move_to_index of every available move as CSR (common.rs:77-86 up to the gather).  The batch is cut into
    // 1 + helpers contiguous ranges; this thread takes the first, a PrepHelper each of the others; the ranges meet in the
    // staging vectors in board order.
    struct PrepRange {
        std::vector<float> scalars;
        std::vector<int64_t> counts;   // moves per board
        std::vector<int32_t> indices;
    };
    std::vector<PrepRange> ranges_ = std::vector<PrepRange>(1);
    std::vector<std::unique_ptr<PrepHelper>> helpers_;

    void prep_range(const B *boards, size_t lo, size_t hi, bool moves, PrepRange &out) {
        const size_t bool_count = input_bool_len(mapper_), bits_bytes = (bool_count + 7) / 8, policy_len = mapper_.policy_len();
        out.scalars.clear();
        out.counts.clear();
        out.indices.clear();
        BitBuffer buffer(bool_count);
        for (size_t bi = lo; bi < hi; bi++) {
            buffer.clear();
            mapper_.encode_input(buffer, out.scalars, boards[bi]);
            if (buffer.len() != bool_count) throw std::logic_error("mapper wrote the wrong number of bools");
            std::copy(buffer.storage().begin(), buffer.storage().begin() + bits_bytes, bits_.begin() + bi * bits_bytes);
            if (!moves) continue;
            const size_t before = out.indices.size();
            bool carried = false;
            if constexpr (has_policy_indices<B>::value) {
                if (const std::vector<int32_t> *idx = boards[bi].policy_indices()) {
                    for (int32_t index : *idx)
                        if (index < 0 || (size_t)index >= policy_len) throw std::out_of_range("policy index out of range");
                    out.indices.insert(out.indices.end(), idx->begin(), idx->end());
                    carried = true;
                }
            }
            if (!carried) {
                auto available = boards[bi].available_moves();
                if (available)
                    for (const auto &mv : *available) {
                        const size_t index = mapper_.move_to_index(boards[bi], mv);
                        if (index >= policy_len) throw std::out_of_range("move_to_index out of range");
                        out.indices.push_back((int32_t)index);
                    }
            }
            out.counts.push_back((int64_t)(out.indices.size() - before));
        }
    }

    // returns bits_bytes; fills bits_, scalars_in_ and (moves) offsets + move_indices_
    size_t prepare(const B *boards, size_t n, bool moves, std::vector<int64_t> *offsets) {
        const size_t parts = std::min(ranges_.size(), std::max<size_t>(1, n / 16));  // (a handful of boards: not worth a hand-over)
        auto cut = [&](size_t k) { return n * k / parts; };
        for (size_t k = 1; k < parts; k++)
            helpers_[k - 1]->start([this, boards, moves, k, lo = cut(k), hi = cut(k + 1)] { prep_range(boards, lo, hi, moves, ranges_[k]); });
        std::exception_ptr first;
        const uint64_t t0 = thread_cpu_ns();
        try {
            prep_range(boards, 0, cut(1), moves, ranges_[0]);
        } catch (...) {
            first = std::current_exception();
        }
        prep_own_cpu_ns += thread_cpu_ns() - t0;
        for (size_t k = 1; k < parts; k++) {  // every helper is waited for, whatever happened: the boards are the caller's
            try {
                helpers_[k - 1]->finish();
            } catch (...) {
                if (!first) first = std::current_exception();
            }
        }
        if (first) std::rethrow_exception(first);
        const uint64_t t1 = thread_cpu_ns();
        scalars_in_.clear();
        if (moves) {
            offsets->assign(1, 0);
            move_indices_.clear();
        }
        for (size_t k = 0; k < parts; k++) {
            const PrepRange &r = ranges_[k];
            scalars_in_.insert(scalars_in_.end(), r.scalars.begin(), r.scalars.end());
            if (!moves) continue;
            move_indices_.insert(move_indices_.end(), r.indices.begin(), r.indices.end());
            for (int64_t c : r.counts) offsets->push_back(offsets->back() + c);
        }
        merge_cpu_ns += thread_cpu_ns() - t1;
        return (input_bool_len(mapper_) + 7) / 8;
    }

    // kz_engine_wait_decoded through the status entry (kz_engine_wait_decoded_status): boards the range fallback re-evaluated
    // (status exactly KZ_BOARD_FELL_BACK: their results are the exact-f32 ones) are counted; any other non-zero status throws —
    // the reference panics on every executor error — naming the boards
    void wait_decoded_checked(int slot, size_t n, const float **values, const float **probs) {
        void *status_view = nullptr;
        kz_check(kz_engine_wait_decoded_status(engine_, slot, values, probs, &status_view));
        const uint8_t *status = static_cast<const uint8_t *>(status_view);
        std::string bad;
        bool nonfinite = false;
        for (size_t b = 0; b < n; b++) {
            if (status[b] == KZ_BOARD_OK) continue;
            if (status[b] == KZ_BOARD_FELL_BACK) {
                fell_back_boards++;
                continue;
            }
            nonfinite = nonfinite || (status[b] & KZ_BOARD_NONFINITE);
            bad += (bad.empty() ? "" : ", ") + std::to_string(b);
        }
        if (bad.empty()) return;
        throw std::runtime_error(std::string("kzhip: ") +
                                 (nonfinite ? "non-finite activation (beyond +-65504 the f16 and split-f16 paths overflow: set_range_fallback(true) "
                                              "re-evaluates such boards in exact f32)"
                                            : "Softmax input sum must be strictly positive (or a move index or symmetry id is out of range)") +
                                 " on boards " + bad + " of the batch");
    }

    // values [n,5] (already tanh / softmax) + probabilities parallel to the move lists -> evaluations
    static std::vector<ZeroEvaluation> assemble_decoded(size_t n, const std::vector<int64_t> &offsets, const float *values,
                                                        const float *probs) {
        std::vector<ZeroEvaluation> out(n);
        for (size_t bi = 0; bi < n; bi++) {
            const float *v = values + bi * 5;
            out[bi].values = ZeroValuesPov{v[0], WDL{v[1], v[2], v[3]}, v[4]};
            out[bi].policy.assign(probs + offsets[bi], probs + offsets[bi + 1]);
        }
        return out;
    }

  public:
    // CPU time this thread has spent inside kz_engine_wait* so far: the HIP runtime polls the event, so an executor
    // thread shows ~100 % CPU however little work it does; (thread CPU - this) is its work
    uint64_t wait_cpu_ns = 0;
    // ... and where the rest goes (measurement, tests/cpp/bench_executor.cpp): this thread's share of a batch's preparation, the
    // merge of the ranges, the engine's submit call (copies into pinned staging + the launch), building the evaluations
    uint64_t prep_own_cpu_ns = 0, merge_cpu_ns = 0, submit_cpu_ns = 0, assemble_cpu_ns = 0;
    // boards the range fallback has re-evaluated in exact f32 so far (set_range_fallback; the device decode's calls count them)
    uint64_t fell_back_boards = 0;
    // cudnn.rs:29-43 (check_graph_shapes: common.rs:165-198)
    // dtype: KZ_DTYPE_F32 / KZ_DTYPE_F16 / KZ_DTYPE_F32_SPLIT16 / KZ_DTYPE_BF16 (f32 tensors like split16, the one-launch ResTower
    // in bf16: f32's range, nothing for set_range_fallback to catch; kz_model_supports_dtype tells whether the model has it)
    HipNetwork(M mapper, std::shared_ptr<const HipModel> model, size_t max_batch_size, int device, int dtype)
        : mapper_(mapper), model_(std::move(model)), max_batch_size_(max_batch_size) {
        const kz_model_info &info = model_->info;
        auto shape = input_full_shape(mapper_);
        if ((size_t)info.input_channels != shape[0] || (size_t)info.board_h != shape[1] || (size_t)info.board_w != shape[2])
            throw std::invalid_argument("Input shape mismatch between model and mapper");
        if ((size_t)info.input_scalar_channels != mapper_.input_scalar_count())
            throw std::invalid_argument("Scalar plane count mismatch between model and mapper");
        if ((size_t)info.policy_len != mapper_.policy_len()) throw std::invalid_argument("Wrong policy shape");
        kz_check(kz_engine_create(model_->get(), device, (int)max_batch_size, dtype, &engine_));
        bits_.resize(max_batch_size * (size_t)info.bits_bytes);
        if (StreamShiftEnv::from_env().automatic) set_position_sample(process_position_sample());
    }
    HipNetwork(HipNetwork &&o) noexcept
        : mapper_(o.mapper_), model_(std::move(o.model_)), engine_(o.engine_), max_batch_size_(o.max_batch_size_),
          bits_(std::move(o.bits_)), scalars_in_(std::move(o.scalars_in_)), next_slot_(o.next_slot_),
          oldest_slot_(o.oldest_slot_), in_flight_(o.in_flight_), device_decode_(o.device_decode_), n_sym_(o.n_sym_),
          sym_rng_(o.sym_rng_), average_(o.average_), sample_(std::move(o.sample_)), ranges_(std::move(o.ranges_)), helpers_(std::move(o.helpers_)), wait_cpu_ns(o.wait_cpu_ns),
          fell_back_boards(o.fell_back_boards) {
        for (int i = 0; i < KZ_ENGINE_SLOTS; i++) {
            pending_boards_[i] = std::move(o.pending_boards_[i]);
            move_offsets_[i] = std::move(o.move_offsets_[i]);
        }
        o.engine_ = nullptr;
    }
    HipNetwork(const HipNetwork &) = delete;
    ~HipNetwork() override { kz_engine_destroy(engine_); }

    size_t max_batch_size() const override { return max_batch_size_; }

    // true: decode_output runs on the GPU (legal-move gather + softmax, tanh, wdl); 0.2 KB instead of 7.5 KB per chess
    // evaluation cross PCIe and this thread does no softmax.  Same results to f32 rounding (device expf/tanhf).
    void set_device_decode(bool on) {
        if (in_flight_ != 0) throw std::logic_error("set_device_decode while batches are in flight");
        if (!on && n_sym_) throw std::logic_error("symmetries inside the engine need the device decode");
        device_decode_ = on;
    }

    // true: a board of an f16 / split16 batch whose activations leave the f16 range is re-evaluated in exact f32 inside the
    // engine (kz_engine_set_range_fallback: a sibling engine, created here) instead of failing the batch; fell_back_boards
    // counts them.  Off by default, like hip.rs's KZ_HIP_RANGE_FALLBACK.  An exact-f32 engine refuses it (the call throws).
    void set_range_fallback(bool on) {
        if (in_flight_ != 0) throw std::logic_error("set_range_fallback while batches are in flight");
        kz_check(kz_engine_set_range_fallback(engine_, on ? KZ_DTYPE_F32 : -1));
    }

    // The shadow audit (kz_engine_set_audit: a second sibling engine, created here): the first `boards` boards of every
    // `period`-th batch of the device decode also run in `dtype` — KZ_DTYPE_F32_SPLIT16 or KZ_DTYPE_F32 — beside the batch and
    // the engine accumulates the deviation; no evaluation changes.  dtype -1 turns it off.  Off by default, like the Rust
    // shim's switch for it.  (A KZ_DTYPE_BF16 network takes either.)  The engine's own dtype, KZ_DTYPE_F16 and a sample larger than min(64, max_batch_size) are refused (throws).
    void set_audit(int dtype, int period = 1, int boards = 16) {
        if (in_flight_ != 0) throw std::logic_error("set_audit while batches are in flight");
        kz_check(kz_engine_set_audit(engine_, dtype, period, boards));
    }
    // what the audit has accumulated so far (kz_engine_audit_stats); reset: zero it afterwards
    kz_audit_stats audit_stats(bool reset = false) {
        kz_audit_stats out;
        kz_check(kz_engine_audit_stats(engine_, &out, reset ? 1 : 0));
        return out;
    }

    // `eval_random_symmetries` (symmetry.rs:18-68) inside the launch: every board of every batch is evaluated under a symmetry
    // drawn from `rng` — the ids RandomSymmetryNetwork<B, HipNetwork> would draw from the same rng — and the engine maps the
    // planes on the way in and the policy indices on the way out (kz_engine_set_symmetries).  This thread then does what it does
    // without symmetries: no board is mapped, no move list regenerated or searched.  Turns the device decode on (the mapped
    // logits never reach the host).  tables: d4_tables(mapper) for Ataxx and Go.
    void set_random_symmetries(const SymmetryTables &tables, std::mt19937_64 rng) {
        if (in_flight_ != 0) throw std::logic_error("set_random_symmetries while batches are in flight");
        if (average_) throw std::logic_error("set_random_symmetries after set_average_symmetries: one or the other");
        if (tables.hw != model_->info.board_h * model_->info.board_w || tables.policy_len != model_->info.policy_len)
            throw std::invalid_argument("symmetry tables of another board or policy");
        kz_check(kz_engine_set_symmetries(engine_, tables.n_sym, tables.square_src.data(), tables.policy_map.data()));
        n_sym_ = tables.n_sym;
        sym_rng_ = rng;
        device_decode_ = true;
    }

    // `AverageSymmetryNetwork` (symmetry.rs:70-124,150-184) inside the engine: every board of every batch is evaluated under
    // ALL symmetries of `tables`, in row order, and values and policy are averaged on the device
    // (kz_engine_submit_packed_decoded_avg) — this thread encodes each board once and gets one result per board.  The engine
    // takes max_batch_size() / n_sym boards per call: evaluate_batch chunks by that, the way the wrapper chunks the mapped
    // boards by the inner network's max_batch_size (:108-113); submit_batch takes at most that many.  max_batch_size() keeps
    // its meaning (the engine's).  Exclusive with set_random_symmetries; turns the device decode on.
    void set_average_symmetries(const SymmetryTables &tables) {
        if (in_flight_ != 0) throw std::logic_error("set_average_symmetries while batches are in flight");
        if (n_sym_ && !average_) throw std::logic_error("set_average_symmetries after set_random_symmetries: one or the other");
        if (tables.hw != model_->info.board_h * model_->info.board_w || tables.policy_len != model_->info.policy_len)
            throw std::invalid_argument("symmetry tables of another board or policy");
        if (tables.n_sym < 1 || (size_t)tables.n_sym > max_batch_size_)
            throw std::invalid_argument("max_batch_size must hold one board under every symmetry");
        kz_check(kz_engine_set_symmetries(engine_, tables.n_sym, tables.square_src.data(), tables.policy_map.data()));
        n_sym_ = tables.n_sym;
        average_ = true;
        device_decode_ = true;
    }

    // evaluate_batch and submit_batch offer the boards they have just packed to `sample` (PositionSample: the first `take`
    // boards of every `period`-th call, a memcpy) — what HipModel::auto_stream_shift profiles the next network on.  One sample
    // for all executors of a process.  Off by default (null turns it off again); KZ_HIP_STREAM_SHIFT=auto turns it on with
    // process_position_sample().
    void set_position_sample(std::shared_ptr<PositionSample> sample) {
        if (sample) sample->bind((size_t)model_->info.bits_bytes, (size_t)model_->info.input_scalar_channels);
        sample_ = std::move(sample);
    }

    // Helper threads for a batch's host work (encode_input, move lists): 0 = all of it on the calling executor thread like
    // the reference; 1 (hip.rs's default) halves what the executor thread does per batch.  Results are identical.
    void set_prep_helpers(size_t n) {
        if (in_flight_ != 0) throw std::logic_error("set_prep_helpers while batches are in flight");
        helpers_.clear();
        for (size_t i = 0; i < n; i++) helpers_.push_back(std::make_unique<PrepHelper>());
        ranges_.assign(n + 1, PrepRange{});
    }
    // CPU time the helper threads have used so far (measurement)
    uint64_t helper_cpu_ns() const {
        uint64_t t = 0;
        for (const auto &h : helpers_) t += h->cpu_ns.load();
        return t;
    }

    // cudnn.rs:55-87
    std::vector<ZeroEvaluation> evaluate_batch(const B *boards, size_t n) override {
        if (n > max_batch_size_) throw std::invalid_argument("batch_size <= max_batch_size");  // assert!, :58
        if (n == 0) return {};
        if (in_flight_ != 0) throw std::logic_error("evaluate_batch while submitted batches are in flight");
        if (average_ && n * (size_t)n_sym_ > max_batch_size_) {  // the engine's limit per averaged call: chunk
            const size_t chunk = max_batch_size_ / (size_t)n_sym_;
            std::vector<ZeroEvaluation> out;
            out.reserve(n);
            for (size_t lo = 0; lo < n; lo += chunk)
                for (auto &ev : evaluate_batch(boards + lo, std::min(chunk, n - lo))) out.push_back(std::move(ev));
            return out;
        }
        const size_t bits_bytes = prepare(boards, n, device_decode_, &move_offsets_[0]);
        offer_sample(bits_bytes, n);
        if (device_decode_) {
            const float *values = nullptr, *probs = nullptr;
            submit_decoded(0, bits_bytes, n);
            const uint64_t w0 = thread_cpu_ns();
            wait_decoded_checked(0, n, &values, &probs);
            wait_cpu_ns += thread_cpu_ns() - w0;
            return assemble_decoded(n, move_offsets_[0], values, probs);
        }
        // kz_engine_eval_packed without its copy into caller buffers: decode reads the pinned staging directly
        const float *scalars = nullptr, *policy = nullptr;
        kz_check(kz_engine_submit_packed(engine_, 0, bits_.data(), bits_bytes, scalars_in_.data(), (int)n));
        const uint64_t w0 = thread_cpu_ns();
        kz_check(kz_engine_wait_view(engine_, 0, &scalars, &policy));
        wait_cpu_ns += thread_cpu_ns() - w0;
        return decode_output(mapper_, boards, n, scalars, policy);
    }

    // ---- asynchronous pair for pipelined_executor_loop (kz_engine_submit_packed / kz_engine_wait) ----
    static constexpr size_t max_in_flight() { return KZ_ENGINE_SLOTS; }
    size_t batches_in_flight() const { return (size_t)in_flight_; }

    // encode + hand the batch to the engine; returns while the GPU works.  The boards are MOVED out of `boards`
    // (decode_output needs their available moves when the results come back); the pointer itself is not retained.
    void submit_batch(B *boards, size_t n) {
        if (n == 0 || n > max_batch_size_) throw std::invalid_argument("0 < batch_size <= max_batch_size");
        if (in_flight_ == KZ_ENGINE_SLOTS) throw std::logic_error("every engine slot is in flight");
        if (average_ && n * (size_t)n_sym_ > max_batch_size_) throw std::invalid_argument("an averaged batch is at most max_batch_size / n_sym boards");
        const size_t bits_bytes = prepare(boards, n, device_decode_, &move_offsets_[next_slot_]);
        offer_sample(bits_bytes, n);
        // the engine copies its inputs to pinned staging before submit returns (include/kz_hip.h)
        if (device_decode_) {
            const uint64_t s0 = thread_cpu_ns();
            submit_decoded(next_slot_, bits_bytes, n);
            submit_cpu_ns += thread_cpu_ns() - s0;
            pending_boards_[next_slot_].clear();  // the move lists are all the decode needs
        } else {
            kz_check(kz_engine_submit_packed(engine_, next_slot_, bits_.data(), bits_bytes, scalars_in_.data(), (int)n));
            pending_boards_[next_slot_].assign(std::make_move_iterator(boards), std::make_move_iterator(boards + n));
        }
        next_slot_ = (next_slot_ + 1) % KZ_ENGINE_SLOTS;
        in_flight_++;
    }

    // results of the OLDEST submitted batch
    std::vector<ZeroEvaluation> wait_batch() {
        if (in_flight_ == 0) throw std::logic_error("wait_batch with nothing in flight");
        const int slot = oldest_slot_;
        oldest_slot_ = (oldest_slot_ + 1) % KZ_ENGINE_SLOTS;
        in_flight_--;
        if (device_decode_) {
            const float *values = nullptr, *probs = nullptr;
            const uint64_t w0 = thread_cpu_ns();
            wait_decoded_checked(slot, move_offsets_[slot].size() - 1, &values, &probs);
            const uint64_t w1 = thread_cpu_ns();
            wait_cpu_ns += w1 - w0;
            auto out = assemble_decoded(move_offsets_[slot].size() - 1, move_offsets_[slot], values, probs);
            assemble_cpu_ns += thread_cpu_ns() - w1;
            return out;
        }
        // decode straight from the engine's pinned staging (valid until the next submit on this slot)
        const float *scalars = nullptr, *policy = nullptr;
        const uint64_t w0 = thread_cpu_ns();
        kz_check(kz_engine_wait_view(engine_, slot, &scalars, &policy));
        wait_cpu_ns += thread_cpu_ns() - w0;
        const std::vector<B> &boards = pending_boards_[slot];
        return decode_output(mapper_, boards.data(), boards.size(), scalars, policy);
    }
};

}  // namespace kz::host
