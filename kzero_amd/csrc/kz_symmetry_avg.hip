// kz_symmetry_avg.hip — `AverageSymmetryNetwork` (rust/kz-core/src/network/symmetry.rs:70-124,150-184) around the unchanged
// network launches: every board of a batch is evaluated under EVERY symmetry of the engine's tables and the decoded values
// and probabilities are averaged.  Two small HBM-side kernels (include/kz_hip.h: the `_avg` entries):
//
//   kz_sym_fan_out   the slot's pinned staging (batch boards, their CSR move lists) -> the VIRTUAL batch in device scratch:
//                    virtual board v = b * n_sym + k is board b under symmetry k (the reference's flat_map order, :98-101) —
//                    bits and scalars replicated n_sym times, ids = k, the move list replicated with
//                    voff[b n + k] = n off[b] + k len_b, voff[n batch] = n total.
//   (the network)    forward_packed on the virtual batch with ids: the encode and the decode apply the tables as they do
//                    for the `_sym` entries; the decode writes virtual values / probabilities to device scratch.
//   kz_sym_average   values[b][j] = (((0 + v_0) + v_1) + ... + v_{n-1}) / n                          (:156-160)
//                    probs[lo_b + i] = ((0 + p_0 / n) + p_1 / n) + ...  in the caller's move order    (:166-176)
//                    all in f32, every division correctly rounded; rows are summed in id order 0 .. n_sym-1.
//
// Nothing here is atomic and no workgroup talks to another: a result is a function of its inputs alone.
#include "kz_kernels.hpp"

namespace kz {
namespace {

constexpr int FAN_THREADS = 256;  // n_sym <= 255 (kz_engine_set_symmetries): one thread per virtual offset of a board
constexpr int AVG_WAVES = 4;

// One workgroup per SOURCE board.  Every staged word of the board is read once (a pinned-host read crosses PCIe) — the
// board's bits, scalars and move indices by one thread each, which then stores the n_sym copies: for a fixed k the
// workgroup's stores are consecutive addresses.  (The CSR offset a board shares with its neighbour is read by both.)
__global__ __launch_bounds__(FAN_THREADS) void kz_sym_fan_out(SymFanOutArgs a) {
    const int b = blockIdx.x, t = threadIdx.x, n = a.n_sym;
    const int64_t lo = a.move_offsets[b], hi = a.move_offsets[b + 1], len = hi - lo;
    const size_t v0 = (size_t)b * n;  // the board's first virtual board
    for (int i = t; i < (int)a.bits_bytes; i += FAN_THREADS) {
        const uint8_t x = a.bits[(size_t)b * a.bits_bytes + i];
        for (int k = 0; k < n; k++) a.v_bits[(v0 + k) * a.bits_bytes + i] = x;
    }
    for (int i = t; i < a.n_scalar; i += FAN_THREADS) {
        const float x = a.scalars[(size_t)b * a.n_scalar + i];
        for (int k = 0; k < n; k++) a.v_scalars[(v0 + k) * a.n_scalar + i] = x;
    }
    for (int64_t i = t; i < len; i += FAN_THREADS) {
        const int32_t x = a.move_indices[lo + i];
        for (int k = 0; k < n; k++) a.v_move_indices[(int64_t)n * lo + k * len + i] = x;
    }
    if (t < n) {
        a.v_sym[v0 + t] = (uint8_t)t;
        a.v_move_offsets[v0 + t] = (int64_t)n * lo + t * len;
    }
    if (b == a.batch - 1 && t == 0) a.v_move_offsets[(size_t)n * a.batch] = (int64_t)n * hi;
    if (b == 0 && t == 0) a.v_error_flag[0] = a.v_error_flag[1] = 0;  // the decode of this batch raises them
    for (int i = t; i < 2 * n; i += FAN_THREADS) a.v_error_flag[ERR_HDR + 2 * v0 + i] = 0;  // ... and its virtual boards' own words (two each): cleared per submit
}

// One WAVE per source board.  Lanes 0..4 reduce the five values; then the lanes stride over the board's moves and each sums
// its move over k ascending.  values / probs / error_flag are the slot's pinned staging: every word written once, by a plain
// store.
__global__ __launch_bounds__(AVG_WAVES * 64) void kz_sym_average(SymAverageArgs a) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int b = blockIdx.x * AVG_WAVES + wave, n = a.n_sym;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        a.error_flag[0] = a.v_error_flag[0];
        a.error_flag[1] = a.v_error_flag[1];
    }
    if (b >= a.batch) return;
    const float nf = (float)n;
    const size_t v0 = (size_t)b * n;
    // the source board's status = the OR over its n virtual boards: the decode's word, and the range check's from either
    // place a virtual board's can be (the stand-alone decode's copy, or the launch's epoch-stamped word)
    if (lane == 0) {
        int dec = 0, range = 0;
        for (int k = 0; k < n; k++) {
            dec |= a.v_error_flag[ERR_HDR + 2 * (v0 + k)];
            range |= a.v_error_flag[ERR_HDR + 2 * (v0 + k) + 1];
            if (a.nonfinite_flag) range |= a.nonfinite_flag[-1 - (int)(v0 + k)] == a.epoch;
        }
        if (dec) a.error_flag[ERR_HDR + 2 * b] = 1;
        if (range) a.error_flag[ERR_HDR + 2 * b + 1] = 1;
    }
    if (lane < 5) {
        float acc = 0.0f;
        for (int k = 0; k < n; k++) acc = acc + a.v_values[(v0 + k) * 5 + lane];
        a.values[(size_t)b * 5 + lane] = __fdiv_rn(acc, nf);
    }
    // the board's own range from its virtual ones: voff[v0] = n lo, voff[v0 + 1] - voff[v0] = len
    const int64_t vlo = a.v_move_offsets[v0], len = a.v_move_offsets[v0 + 1] - vlo, lo = vlo / n;
    for (int64_t i = lane; i < len; i += 64) {
        float acc = 0.0f;
        for (int k = 0; k < n; k++) acc = acc + __fdiv_rn(a.v_probs[vlo + k * len + i], nf);
        a.probs[lo + i] = acc;
    }
}

}  // namespace

void launch_sym_fan_out(const SymFanOutArgs &a, hipStream_t stream) {
    kz_sym_fan_out<<<a.batch, FAN_THREADS, 0, stream>>>(a);
}

void launch_sym_average(const SymAverageArgs &a, hipStream_t stream) {
    kz_sym_average<<<(a.batch + AVG_WAVES - 1) / AVG_WAVES, AVG_WAVES * 64, 0, stream>>>(a);
}

}  // namespace kz
