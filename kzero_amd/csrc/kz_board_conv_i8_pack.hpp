// kz_board_conv_i8_pack.hpp — the int8 weight stream of kz_board_conv_i8 (kz_board_conv_i8.hip), plain C++ with no HIP in it:
// the kernel's translation unit and the stand-alone packing test (tests/cpp/test_board_conv_i8_pack.cpp) include it.
#pragma once
#include <cstddef>
#include <cstdint>

namespace kz {

// wq [cout][cin][9] int8 -> [quarter = cout8 / 64][chunk = cin8 / 128][tap 9][ks 2][nt 4][lane 64][16], the order the kernel
// streams it in: byte j of lane (fr = lane % 16, kq = lane / 16) is
//   wq[oc = 64 quarter + 16 nt + fr][channel = 128 chunk + 64 (kq & 1) + 32 ks + 16 (kq >> 1) + j][tap]
// — the A fragment of v_mfma_i32_16x16x64_i8 for the sixteen bytes the same lane group reads of a pixel row's chunk (plane
// kq & 1, byte 32 ks + 16 (kq >> 1) of the plane) —, 0 for a widened output or input channel (oc >= cout, channel >= cin).
// cout8 is a multiple of 64, cin8 of 128; dst holds 9 * cin8 * cout8 bytes.
inline void board_conv_i8_pack_weights_host(const int8_t *wq, int cout, int cin, int cout8, int cin8, int8_t *dst) {
    const int chunks = cin8 / 128, quarters = cout8 / 64;
    size_t o = 0;
    for (int nq = 0; nq < quarters; nq++)
        for (int chunk = 0; chunk < chunks; chunk++)
            for (int tap = 0; tap < 9; tap++)
                for (int ks = 0; ks < 2; ks++)
                    for (int nt = 0; nt < 4; nt++)
                        for (int lane = 0; lane < 64; lane++)
                            for (int j = 0; j < 16; j++) {
                                const int kq = lane >> 4;
                                const int oc = 64 * nq + 16 * nt + (lane & 15);
                                const int ch = 128 * chunk + 64 * (kq & 1) + 32 * ks + 16 * (kq >> 1) + j;
                                dst[o++] = oc < cout && ch < cin ? wq[((size_t)oc * cin + ch) * 9 + tap] : (int8_t)0;
                            }
}

}  // namespace kz
