// kz_range_profile.hip — the range profile's two kernels (kz_model_range_profile, kz_model_range_histogram, include/kz_hip.h):
// max |x| of one stored tower tensor, per board, and the tensor's binade counts, in exact f32.
//
//   kz_range_absmax     one 256-thread workgroup per board over the board's hw rows of `channels` real f32 values (row stride
//                       cp floats, rows 128-byte aligned: 16-byte loads); one f32 per board out
//   kz_range_histogram  the same rows of all boards, grid-strided in 16-byte chunks; each wave bins (range_bin) into LDS
//                       histograms of its own — SUB copies, chosen by lane, so that the 64 lanes of a wave that hit one bin
//                       queue four deep, not 64 —, the workgroup adds its non-empty bins to the 96 global counters
//
// The maximum is taken over `bits & 0x7fffffff` as unsigned: a NaN sorts above inf, and anything above inf's pattern is
// clamped to it, so a board with any non-finite value reports +inf.  max is order-independent and nothing is shared between
// workgroups: the result does not depend on scheduling.  HBM-bound (4 B per element, read once).
// The histogram's counters are integers added with atomics: sums commute, so neither does it.
#include <algorithm>

#include "kz_kernels.hpp"

namespace kz {

__global__ __launch_bounds__(256) void kz_range_absmax(const float *__restrict__ x, int hw, int channels, int cp,
                                                       float *__restrict__ out) {
    const int b = blockIdx.x;
    const uint4 *rows = reinterpret_cast<const uint4 *>(x + (size_t)b * hw * cp);
    const int chunks = cp / 4, used = (channels + 3) / 4;  // 16-byte chunks per row, and those that hold a real channel
    unsigned m = 0;
    for (int i = threadIdx.x; i < hw * used; i += 256) {
        const int r = i / used, g = i - r * used;
        const uint4 v = rows[r * chunks + g];
        const int left = channels - g * 4;  // real channels in this chunk: >= 1
        m = max(m, v.x & 0x7fffffffu);
        if (left > 1) m = max(m, v.y & 0x7fffffffu);
        if (left > 2) m = max(m, v.z & 0x7fffffffu);
        if (left > 3) m = max(m, v.w & 0x7fffffffu);
    }
    m = min(m, 0x7f800000u);
#pragma unroll
    for (int off = 32; off; off >>= 1) m = max(m, (unsigned)__shfl_xor((int)m, off));
    __shared__ unsigned part[4];
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) out[b] = __uint_as_float(max(max(part[0], part[1]), max(part[2], part[3])));
}

// copy stride 97 words: the SUB copies of one bin lie in different banks
constexpr int HIST_SUB = 16, HIST_STRIDE = RANGE_BINS + 1;

__global__ __launch_bounds__(256) void kz_range_histogram(const float *__restrict__ x, int rows_n, int channels, int cp,
                                                          unsigned long long *__restrict__ hist) {
    __shared__ unsigned part[4 * HIST_SUB * HIST_STRIDE];
    for (int i = threadIdx.x; i < 4 * HIST_SUB * HIST_STRIDE; i += 256) part[i] = 0;
    __syncthreads();
    unsigned *mine = part + ((threadIdx.x >> 6) * HIST_SUB + (threadIdx.x & (HIST_SUB - 1))) * HIST_STRIDE;
    const uint4 *rows = reinterpret_cast<const uint4 *>(x);
    const int chunks = cp / 4, used = (channels + 3) / 4;
    const size_t total = (size_t)rows_n * used;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const size_t r = i / used;
        const int g = (int)(i - r * used);
        const uint4 v = rows[r * chunks + g];
        const int left = channels - g * 4;  // real channels in this chunk: >= 1
        atomicAdd(mine + range_bin(v.x), 1u);
        if (left > 1) atomicAdd(mine + range_bin(v.y), 1u);
        if (left > 2) atomicAdd(mine + range_bin(v.z), 1u);
        if (left > 3) atomicAdd(mine + range_bin(v.w), 1u);
    }
    __syncthreads();
    if (threadIdx.x < RANGE_BINS) {
        unsigned n = 0;
        for (int c = 0; c < 4 * HIST_SUB; c++) n += part[c * HIST_STRIDE + threadIdx.x];
        if (n) atomicAdd(hist + threadIdx.x, (unsigned long long)n);
    }
}

void launch_range_absmax(const float *x, int boards, int hw, int channels, int cp, float *out, hipStream_t stream) {
    kz_range_absmax<<<boards, 256, 0, stream>>>(x, hw, channels, cp, out);
}

void launch_range_histogram(const float *x, int boards, int hw, int channels, int cp, unsigned long long *hist, hipStream_t stream) {
    // 8 chunks of 16 bytes per thread, at most 1024 workgroups (a workgroup's count stays far below 2^32)
    const size_t total = (size_t)boards * hw * ((channels + 3) / 4);
    const int grid = (int)std::min<size_t>((total + 2047) / 2048, 1024);
    kz_range_histogram<<<grid, 256, 0, stream>>>(x, boards * hw, channels, cp, hist);
}

}  // namespace kz
