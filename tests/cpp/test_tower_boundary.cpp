// Conv A's epilogue of the chess f16 tower: ReLU on the f32 bits and then the conversion to f16 (relu4, to_h4) against the
// conversion first and the ReLU on the packed f16 bits (kz_tower_boundary.hpp, relu_f16_bits) — the same bits for every
// input.  Host build of the header's own functions; the conversion is the compiler's round-to-nearest-even f32 -> f16.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>

#include "../../kzero_amd/csrc/kz_tower_boundary.hpp"

static uint16_t to_f16_bits(uint32_t f32_bits) {
    float f;
    std::memcpy(&f, &f32_bits, 4);
    const _Float16 h = (_Float16)f;
    uint16_t b;
    std::memcpy(&b, &h, 2);
    return b;
}

static uint32_t f16_to_f32_bits(uint16_t h_bits) {
    _Float16 h;
    std::memcpy(&h, &h_bits, 2);
    const float f = (float)h;
    uint32_t b;
    std::memcpy(&b, &f, 4);
    return b;
}

static unsigned long long checked = 0, failed = 0;

// two inputs at a time, so that both halves of the packed max are exercised with unrelated neighbours
static void check(uint32_t a, uint32_t b) {
    const uint16_t ra = to_f16_bits(kz::boundary::relu_f32_bits(a)), rb = to_f16_bits(kz::boundary::relu_f32_bits(b));
    const kz::boundary::s16x2 packed = {(short)to_f16_bits(a), (short)to_f16_bits(b)};
    const kz::boundary::s16x2 r = kz::boundary::relu_f16_bits(packed);
    checked += 2;
    if ((uint16_t)r[0] != ra || (uint16_t)r[1] != rb) {
        if (failed++ < 10)
            std::printf("MISMATCH f32 %08x %08x: relu then convert %04x %04x, convert then relu %04x %04x\n", a, b, ra, rb,
                        (unsigned)(uint16_t)r[0], (unsigned)(uint16_t)r[1]);
    }
}

int main() {
    // every f16 value, its f32 neighbours, and the rounding boundaries to the next f16 with their f32 neighbours; both signs
    // come with the patterns.  (NaN patterns included: every f16 NaN payload widened, plus f32-only payloads below.)
    uint32_t prev = 0x3f800000u;
    for (uint32_t h = 0; h < 0x10000u; h++) {
        const uint32_t f = f16_to_f32_bits((uint16_t)h);
        const uint32_t next = f16_to_f32_bits((uint16_t)(h + 1));
        for (int d = -2; d <= 2; d++) {
            check(f + (uint32_t)d, prev);
            check(prev, f + (uint32_t)d);
            // the midpoint of two adjacent f16 magnitudes (the tie of round-to-nearest-even) and its neighbours
            if ((h & 0x7fffu) < 0x7bffu) check((uint32_t)(((uint64_t)f + next) / 2) + (uint32_t)d, f);
        }
        prev = f ^ 0x80000000u;
    }
    // f32 corner patterns: zeros, the smallest and largest subnormals and normals, the f16 overflow threshold, infinities,
    // quiet and signalling NaNs of both signs, payloads that do not survive the narrowing
    const uint32_t corners[] = {0x00000000u, 0x80000000u, 0x00000001u, 0x80000001u, 0x007fffffu, 0x807fffffu, 0x00800000u,
                                0x80800000u, 0x33000000u, 0xb3000000u, 0x33000001u, 0xb3000001u, 0x32ffffffu, 0xb2ffffffu,
                                0x33800000u, 0xb3800000u, 0x38800000u, 0xb8800000u, 0x387fffffu, 0xb87fffffu, 0x477fe000u,
                                0xc77fe000u, 0x477fefffu, 0xc77fefffu, 0x477ff000u, 0xc77ff000u, 0x47800000u, 0xc7800000u,
                                0x7f7fffffu, 0xff7fffffu, 0x7f800000u, 0xff800000u, 0x7fc00000u, 0xffc00000u, 0x7f800001u,
                                0xff800001u, 0x7fa00000u, 0xffa00000u, 0x7fffffffu, 0xffffffffu, 0x7f801fffu, 0xff801fffu};
    for (uint32_t a : corners)
        for (uint32_t b : corners) check(a, b);
    // random f32 bit patterns
    std::mt19937_64 rng(20250611);
    for (int i = 0; i < 20000000; i++) {
        const uint64_t r = rng();
        check((uint32_t)r, (uint32_t)(r >> 32));
    }
    std::printf("%llu values checked, %llu mismatches\n", checked, failed);
    if (failed == 0) std::printf("tower boundary relu tests ok\n");
    return failed == 0 ? 0 : 1;
}
