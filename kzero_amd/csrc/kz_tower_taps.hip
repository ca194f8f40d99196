// kz_tower_taps.hip — the per-site error of a one-launch tower (kz_model_error_profile, include/kz_hip.h): kz_tap_deviation
// reduces one site's tap tensor (the tap instances of kz_tower.hip, kz_tower_pairs.hpp and kz_tower_f32.hip write them:
// kz_kernels.hpp, TapOut) against the exact-f32 tensor of the same site to one TapDeviation record.
//
//   a = the tap's element as f32: f32 as it is, f16 / bf16 widened (exact), a pair as (float)hi + (float)lo
//   r = the reference's f32 value, rows of ref_ld floats (the per-layer engine's padded NHWC rows, or an f32 tap)
//   finite a and r:  max |a - r|, sum (a - r)^2, sum r^2, max |r|, count;  else: nonfinite
//
// Grid-strided over chunks of eight channels of a row — one 16-byte load of a 16-bit tap, two of an f32 one and of the
// reference —; a lane keeps its sums and its maxima in f64 (the difference of two f32 values is exact in f64 unless their
// exponents are more than 29 apart, so max |a - r| is what a host computes in f64 from the same tensors), a wave reduces
// with shuffles, and lane 0 adds the wave's record to the site's with atomics whose result nobody reads (profile_flush's
// rule, kz_tower_f32.hip): f64 adds for the sums, integer adds for the counts, a 64-bit integer max on the bit pattern of a
// non-negative f64 for the maxima.  The maxima and the counts do not depend on the order of the waves; the f64 sums do in
// their last bits (exact where every square is an integer below 2^53).  Bandwidth-bound: every byte is read once.
//
// TapFormat::i8 (kz_model_int8_error_profile): the tap is an int8 image of an int8 tower, eight channels one 8-byte load,
// a = (float)q * 2^e_s (exact); q = -128 — the fill, which the contract never stores — counts as non-finite.  The same pass
// counts |q| == 127 (at_clamp) and finite r with |r| * 2^-e_s >= 127.5 (ref_beyond: what an ideal int8 image of the exact
// network would clamp, rne(127.5) = 128) into the two integers behind the site's records.
#include <algorithm>

#include "kz_kernels.hpp"

namespace kz {

typedef _Float16 h16;
typedef h16 h16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

namespace {

template <TapFormat F>
__device__ __forceinline__ void tap_chunk(const unsigned char *__restrict__ tap, size_t lo_bytes, size_t elem, float (&a)[8]) {
    if constexpr (F == TapFormat::f32) {
        const f32x4 v0 = *reinterpret_cast<const f32x4 *>(tap + elem * 4), v1 = *reinterpret_cast<const f32x4 *>(tap + elem * 4 + 16);
#pragma unroll
        for (int j = 0; j < 4; j++) {
            a[j] = v0[j];
            a[4 + j] = v1[j];
        }
    } else if constexpr (F == TapFormat::i8) {  // q as a float, unscaled; -128 as NaN
        const uint2 v = *reinterpret_cast<const uint2 *>(tap + elem);
        const unsigned w[2] = {v.x, v.y};
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const int q = (int)(signed char)((w[j >> 2] >> (8 * (j & 3))) & 0xffu);
            a[j] = q == -128 ? __uint_as_float(0x7fc00000u) : (float)q;
        }
    } else if constexpr (F == TapFormat::bf16) {  // (a bf16 value is the upper half of its f32)
        const uint4 v = *reinterpret_cast<const uint4 *>(tap + elem * 2);
        const unsigned w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < 4; j++) {
            a[2 * j] = __uint_as_float(w[j] << 16);
            a[2 * j + 1] = __uint_as_float(w[j] & 0xffff0000u);
        }
    } else {
        const h16x8 hi = *reinterpret_cast<const h16x8 *>(tap + elem * 2);
#pragma unroll
        for (int j = 0; j < 8; j++) a[j] = (float)hi[j];
        if constexpr (F == TapFormat::split16) {
            const h16x8 lo = *reinterpret_cast<const h16x8 *>(tap + lo_bytes + elem * 2);
#pragma unroll
            for (int j = 0; j < 8; j++) a[j] += (float)lo[j];
        }
    }
}

template <TapFormat F>
__global__ __launch_bounds__(256) void kz_tap_deviation(const unsigned char *__restrict__ tap, size_t lo_bytes, int tap_ld,
                                                        const float *__restrict__ ref, int ref_ld, size_t rows, int channels,
                                                        TapDeviation *__restrict__ out, float scale = 1.0f, float inv_scale = 1.0f,
                                                        unsigned long long *__restrict__ clamp_counts = nullptr) {
    const int used = (channels + 7) / 8;  // chunks of a row that hold a real channel
    const size_t total = rows * used;
    double sum_err = 0.0, sum_ref = 0.0;
    double max_err = 0.0, max_ref = 0.0;
    unsigned count = 0, nonfinite = 0;  // (a lane sees far fewer than 2^32 elements: launch_tap_deviation's grid)
    unsigned at_clamp = 0, ref_beyond = 0;  // (TapFormat::i8 only)
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (size_t)gridDim.x * 256) {
        const size_t row = i / used;
        const int g = (int)(i - row * used), left = channels - g * 8;  // real channels in this chunk: >= 1
        float a[8];
        tap_chunk<F>(tap, lo_bytes, row * tap_ld + g * 8, a);
        const float *rp = ref + row * ref_ld + g * 8;
        const f32x4 r0 = *reinterpret_cast<const f32x4 *>(rp), r1 = *reinterpret_cast<const f32x4 *>(rp + 4);
#pragma unroll
        for (int j = 0; j < 8; j++) {
            if (j >= left) break;
            const float r = j < 4 ? r0[j] : r1[j - 4];
            if constexpr (F == TapFormat::i8) {
                at_clamp += fabsf(a[j]) == 127.0f;
                ref_beyond += (__float_as_uint(r) & 0x7f800000u) != 0x7f800000u && fabsf(r) * inv_scale >= 127.5f;
                a[j] *= scale;
            }
            // finite: the exponent field is not all ones
            const bool finite = (__float_as_uint(a[j]) & 0x7f800000u) != 0x7f800000u && (__float_as_uint(r) & 0x7f800000u) != 0x7f800000u;
            if (!finite) {
                nonfinite++;
                continue;
            }
            const double dd = (double)a[j] - (double)r;
            max_err = fmax(max_err, fabs(dd));
            max_ref = fmax(max_ref, fabs((double)r));
            sum_err += dd * dd;
            sum_ref += (double)r * (double)r;
            count++;
        }
    }
#pragma unroll
    for (int off = 32; off; off >>= 1) {
        sum_err += __shfl_xor(sum_err, off);
        sum_ref += __shfl_xor(sum_ref, off);
        max_err = fmax(max_err, __shfl_xor(max_err, off));
        max_ref = fmax(max_ref, __shfl_xor(max_ref, off));
        count += __shfl_xor(count, off);
        nonfinite += __shfl_xor(nonfinite, off);
        if constexpr (F == TapFormat::i8) {
            at_clamp += __shfl_xor(at_clamp, off);
            ref_beyond += __shfl_xor(ref_beyond, off);
        }
    }
    if ((threadIdx.x & 63) == 0) {
        if (count) {
            atomicMax(&out->max_abs_err_bits, (unsigned long long)__double_as_longlong(max_err));
            atomicMax(&out->max_abs_ref_bits, (unsigned long long)__double_as_longlong(max_ref));
            atomicAdd(&out->sum_sq_err, sum_err);
            atomicAdd(&out->sum_sq_ref, sum_ref);
            atomicAdd(&out->count, (unsigned long long)count);
        }
        if (nonfinite) atomicAdd(&out->nonfinite, (unsigned long long)nonfinite);
        if constexpr (F == TapFormat::i8) {
            if (at_clamp) atomicAdd(&clamp_counts[0], (unsigned long long)at_clamp);
            if (ref_beyond) atomicAdd(&clamp_counts[1], (unsigned long long)ref_beyond);
        }
    }
}

}  // namespace

void launch_tap_deviation(const void *tap, TapFormat format, size_t lo_bytes, int tap_ld, const float *ref, int ref_ld, size_t rows,
                          int channels, TapDeviation *out, hipStream_t stream) {
    // 8 chunks per thread, at most 2048 workgroups
    const size_t total = rows * ((channels + 7) / 8);
    if (!total) return;
    const int grid = (int)std::min<size_t>((total + 2047) / 2048, 2048);
    const unsigned char *t = static_cast<const unsigned char *>(tap);
    switch (format) {
        case TapFormat::f32: kz_tap_deviation<TapFormat::f32><<<grid, 256, 0, stream>>>(t, lo_bytes, tap_ld, ref, ref_ld, rows, channels, out); break;
        case TapFormat::f16: kz_tap_deviation<TapFormat::f16><<<grid, 256, 0, stream>>>(t, lo_bytes, tap_ld, ref, ref_ld, rows, channels, out); break;
        case TapFormat::split16: kz_tap_deviation<TapFormat::split16><<<grid, 256, 0, stream>>>(t, lo_bytes, tap_ld, ref, ref_ld, rows, channels, out); break;
        case TapFormat::bf16: kz_tap_deviation<TapFormat::bf16><<<grid, 256, 0, stream>>>(t, lo_bytes, tap_ld, ref, ref_ld, rows, channels, out); break;
        case TapFormat::i8: break;  // (launch_tap_deviation_i8: it needs the site's exponent and the record's two counts)
    }
}

void launch_tap_deviation_i8(const void *tap, int tap_ld, int exponent, const float *ref, int ref_ld, size_t rows, int channels,
                             Int8SiteDeviation *out, hipStream_t stream) {
    const size_t total = rows * ((channels + 7) / 8);
    if (!total) return;
    const int grid = (int)std::min<size_t>((total + 2047) / 2048, 2048);
    kz_tap_deviation<TapFormat::i8><<<grid, 256, 0, stream>>>(static_cast<const unsigned char *>(tap), 0, tap_ld, ref, ref_ld, rows, channels,
                                                              &out->image, ldexpf(1.0f, exponent), ldexpf(1.0f, -exponent), &out->at_clamp);
}

}  // namespace kz
