// kz_tower_boundary.hpp — the layer boundary of the line-tile instances of kz_tower_resident (kz_tower.hip), part 1: what
// stands at namespace scope and compiles for the host as well (tests/cpp/test_tower_boundary.cpp).  Part 2,
// kz_tower_boundary_body.hpp, is the k-loop and the epilogue and is included inside the kernel's body.
#pragma once
#include <cstdint>

#include "kz_tower_mfma_order.hpp"  // the order of a k-step's MFMAs, which part 2 (kz_tower_boundary_body.hpp) walks

#ifdef __HIP__
#define KZ_BOUNDARY_FN __host__ __device__ inline
#else
#define KZ_BOUNDARY_FN inline
#endif

namespace kz {
namespace boundary {

// ReLU of packed f16 values on their bit patterns: a signed 16-bit max with 0 per value (v_pk_max_i16, two per instruction).
//
// Conv A's epilogue is relu(v) -> f16.  The tower's relu4 works on the f32 bit pattern, b > 0 ? b : 0 as int32: every value
// with the sign bit set (negative numbers, -0, -inf, a NaN with the sign bit) becomes +0 and every other pattern passes
// unchanged, +NaN included.  Converting first and clamping the f16 pattern the same way gives the same bits for every input:
//   * sign bit clear: the conversion sees the same f32 either way and its result keeps the clear sign (a positive number
//     rounds to a positive number, +0 or +inf; +NaN stays a NaN with the sign clear), so the 16-bit max passes it on — unless
//     it is the pattern 0, which max(0, 0) leaves at 0;
//   * sign bit set: relu4 gives +0, which converts to 0x0000.  Converted first, the f16 keeps the set sign (round-to-nearest
//     never changes a sign: -tiny goes to -0, -huge to -inf, a NaN keeps its sign bit), so as int16 it is negative and the
//     max gives 0x0000.
// The conversion's rounding is the same instruction on the same operand in both orders, so nothing else can differ.
typedef short s16x2 __attribute__((ext_vector_type(2)));  // the bit patterns of two f16 values
KZ_BOUNDARY_FN s16x2 relu_f16_bits(s16x2 b) { return __builtin_elementwise_max(b, s16x2{0, 0}); }

// relu4's element: ReLU on the f32 bit pattern (negative floats are negative integers)
KZ_BOUNDARY_FN uint32_t relu_f32_bits(uint32_t b) { return (int32_t)b > 0 ? b : 0u; }

}  // namespace boundary
}  // namespace kz
