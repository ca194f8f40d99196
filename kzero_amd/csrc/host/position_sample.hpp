// position_sample.hpp — `PositionSample`: the most recent packed boards a process's executors have evaluated, kept for the
// range profile that chooses a network's stream shift (HipModel::auto_stream_shift, KZ_HIP_STREAM_SHIFT=auto).
//
// The quantity the profile measures is a maximum — a tail statistic — so the sample wants many positions, and the positions
// a new network will meet are best guessed by the ones the previous network has just met.  offer() keeps the first `take`
// boards of every `period`-th call — the shadow audit's deterministic prefix rule: no random numbers, a
// memcpy of `take` boards — in a ring of `capacity` boards; snapshot() copies the ring out, oldest board first.
// ONE instance serves all executors of a process (every member function takes the lock): the model is then shifted once.
// A k per executor thread would mean a device weight copy per thread.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <mutex>
#include <stdexcept>
#include <vector>

namespace kz::host {

class PositionSample {
  public:
    struct Snapshot {
        std::vector<uint8_t> bits;   // [boards][bits_bytes], oldest first
        std::vector<float> scalars;  // [boards][n_scalar]
        size_t boards = 0, bits_bytes = 0, n_scalar = 0;
    };

    explicit PositionSample(size_t capacity, size_t period = 1, size_t take = 16) : capacity_(capacity), period_(period), take_(take) {
        if (capacity < 1 || period < 1 || take < 1) throw std::invalid_argument("PositionSample: capacity, period and take must be positive");
    }
    PositionSample(const PositionSample &) = delete;
    PositionSample &operator=(const PositionSample &) = delete;

    // The shape of a packed board (HipNetwork::set_position_sample calls it with its model's).  A sample holds one shape:
    // boards of another one (another game) empty it.
    void bind(size_t bits_bytes, size_t n_scalar) {
        std::lock_guard<std::mutex> l(m_);
        if (bound_ && bits_bytes == bits_bytes_ && n_scalar == n_scalar_) return;
        bound_ = true;
        bits_bytes_ = bits_bytes;
        n_scalar_ = n_scalar;
        bits_.assign(capacity_ * bits_bytes, 0);
        scalars_.assign(capacity_ * n_scalar, 0.0f);
        head_ = size_ = 0;
    }

    // `batch` packed boards as an engine takes them (bits: `stride` bytes apart, scalars: n_scalar floats each): the first
    // min(take, batch) of every period-th call are kept, the oldest boards make room.
    void offer(const uint8_t *bits, size_t stride, const float *scalars, size_t batch) {
        std::lock_guard<std::mutex> l(m_);
        if (!bound_) throw std::logic_error("PositionSample::offer before bind");
        if (calls_++ % period_ != 0) return;
        const size_t n = std::min(take_, batch);
        for (size_t b = 0; b < n; b++) {
            const size_t at = (head_ + size_) % capacity_;
            if (bits_bytes_) std::memcpy(bits_.data() + at * bits_bytes_, bits + b * stride, bits_bytes_);
            if (n_scalar_) std::memcpy(scalars_.data() + at * n_scalar_, scalars + b * n_scalar_, n_scalar_ * sizeof(float));
            if (size_ < capacity_) size_++;
            else head_ = (head_ + 1) % capacity_;
        }
    }

    Snapshot snapshot() const {
        std::lock_guard<std::mutex> l(m_);
        Snapshot s;
        s.boards = size_;
        s.bits_bytes = bits_bytes_;
        s.n_scalar = n_scalar_;
        s.bits.resize(size_ * bits_bytes_);
        s.scalars.resize(size_ * n_scalar_);
        for (size_t i = 0; i < size_; i++) {
            const size_t at = (head_ + i) % capacity_;
            if (bits_bytes_) std::memcpy(s.bits.data() + i * bits_bytes_, bits_.data() + at * bits_bytes_, bits_bytes_);
            if (n_scalar_) std::memcpy(s.scalars.data() + i * n_scalar_, scalars_.data() + at * n_scalar_, n_scalar_ * sizeof(float));
        }
        return s;
    }

    size_t size() const {
        std::lock_guard<std::mutex> l(m_);
        return size_;
    }
    size_t capacity() const { return capacity_; }

  private:
    const size_t capacity_, period_, take_;
    mutable std::mutex m_;
    bool bound_ = false;
    size_t bits_bytes_ = 0, n_scalar_ = 0, head_ = 0, size_ = 0, calls_ = 0;
    std::vector<uint8_t> bits_;
    std::vector<float> scalars_;
};

}  // namespace kz::host
