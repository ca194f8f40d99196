// kz_range_profile.hip — the range profile's one kernel (kz_model_range_profile, include/kz_hip.h): max |x| of one stored
// tower tensor, per board, in exact f32.
//
//   kz_range_absmax    one 256-thread workgroup per board over the board's hw rows of `channels` real f32 values (row stride
//                      cp floats, rows 128-byte aligned: 16-byte loads); one f32 per board out
//
// The maximum is taken over `bits & 0x7fffffff` as unsigned: a NaN sorts above inf, and anything above inf's pattern is
// clamped to it, so a board with any non-finite value reports +inf.  max is order-independent and nothing is shared between
// workgroups: the result does not depend on scheduling.  HBM-bound (4 B per element, read once).
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

void launch_range_absmax(const float *x, int boards, int hw, int channels, int cp, float *out, hipStream_t stream) {
    kz_range_absmax<<<boards, 256, 0, stream>>>(x, hw, channels, cp, out);
}

}  // namespace kz
