// The int8 weight stream of kz_board_conv_i8 (kzero_amd/csrc/kz_board_conv_i8_pack.hpp) against a direct statement of the
// fragment assignment, written from the kernel's reads and not from the packer's loops: for every (oc, channel, tap) of the
// widened convolution, WHERE in the stream the kernel finds it.  Every weight must land there exactly once, every byte of the
// stream must be claimed exactly once, and the widened channels must be zero.  Stand-alone (its own main), built with
// -fsanitize=address,undefined by tests/test_board_conv_i8_pack_cpp.py; no GPU.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../kzero_amd/csrc/kz_board_conv_i8_pack.hpp"

// The kernel: workgroup quarter nq owns output channels [64 nq, 64 nq + 64); per chunk of 128 input channels and tap it
// issues two k-steps; in k-step ks tile column nt's A fragment gives lane (fr, kq) the row oc = 64 nq + 16 nt + fr and the
// sixteen bytes a B lane of the same kq reads from the LDS image: plane kq & 1 (64 channels a plane), byte 32 ks + 16 (kq >> 1)
// of the plane's row.  The stream is read in that order, 16 bytes a lane, 64 lanes, 4 tile columns a k-step.
static size_t where(int oc, int ch, int tap, int cin8) {
    const int nq = oc / 64, nt = (oc % 64) / 16, fr = oc % 16;
    const int chunk = ch / 128, c = ch % 128;
    const int plane = c / 64, in_plane = c % 64;
    const int ks = in_plane / 32, half = (in_plane % 32) / 16, j = in_plane % 16;
    const int kq = plane | (half << 1);
    const int lane = kq * 16 + fr;
    const size_t kstep = ((size_t)(nq * (cin8 / 128) + chunk) * 9 + tap) * 2 + ks;
    return ((kstep * 4 + nt) * 64 + lane) * 16 + j;
}

static int run(int cout, int cin) {
    const int cout8 = (cout + 127) / 128 * 128, cin8 = (cin + 127) / 128 * 128;
    std::vector<int8_t> wq((size_t)cout * cin * 9);
    uint32_t x = 12345u + (uint32_t)cout * 131u + (uint32_t)cin;
    for (auto &v : wq) {  // non-zero everywhere: a weight that lands nowhere, or twice, shows
        x = x * 1664525u + 1013904223u;
        const int r = (int)((x >> 16) % 254) - 127;  // -127 .. 126
        v = (int8_t)(r == 0 ? 127 : r);
    }
    std::vector<int8_t> packed((size_t)9 * cin8 * cout8, (int8_t)0x55);
    kz::board_conv_i8_pack_weights_host(wq.data(), cout, cin, cout8, cin8, packed.data());
    std::vector<uint8_t> claimed(packed.size(), 0);
    for (int oc = 0; oc < cout8; oc++)
        for (int ch = 0; ch < cin8; ch++)
            for (int tap = 0; tap < 9; tap++) {
                const size_t at = where(oc, ch, tap, cin8);
                if (at >= packed.size()) return printf("FAIL %dx%d: (%d, %d, %d) beyond the stream\n", cout, cin, oc, ch, tap), 1;
                if (claimed[at]++) return printf("FAIL %dx%d: byte %zu claimed twice\n", cout, cin, at), 1;
                const int8_t want = oc < cout && ch < cin ? wq[((size_t)oc * cin + ch) * 9 + tap] : (int8_t)0;
                if (packed[at] != want)
                    return printf("FAIL %dx%d: (oc %d, channel %d, tap %d) at byte %zu is %d, not %d\n", cout, cin, oc, ch, tap, at, packed[at], want), 1;
            }
    for (size_t i = 0; i < claimed.size(); i++)
        if (claimed[i] != 1) return printf("FAIL %dx%d: byte %zu of the stream belongs to no weight\n", cout, cin, i), 1;
    return 0;
}

int main() {
    const int shapes[][2] = {{128, 128}, {256, 256}, {192, 192}, {64, 64}, {384, 384}, {96, 96}, {1, 1}, {130, 70}};
    int n = 0;
    for (auto &s : shapes) {
        if (run(s[0], s[1])) return 1;
        n++;
    }
    printf("board_conv_i8 pack tests ok: %d shapes\n", n);
    return 0;
}
