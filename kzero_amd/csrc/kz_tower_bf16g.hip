// kz_tower_bf16g.hip — the BF = true instances of kz_tower_pairs.hpp: the one-launch tower of kz_tower_f16g.hip with bf16 as the
// element of its images, weight fragments and MFMAs (v_mfma_f32_16x16x32_bf16, f32 accumulation; bias, ReLU, residual add and
// the final BN in f32) and f32 tensors at its boundary — dtype 3's "tower_resident_bf16g[+heads]": f32's range at the f16
// rate, 8 significant bits.  Same shapes, tiles and choice among them as the plain-f16 family (64 .. 512 channels on small
// boards, the wide tiles at 128 / 192 channels); the conv heads' tail inside the launch is exact f32.  The kernel's body is in
// kz_tower_pairs.hpp; this file holds this family's instances.
#include "kz_tower_pairs.hpp"

namespace kz {

void launch_tower_bf16(const Tower32Args &t, hipStream_t stream) {
    int nt = 0, grid = 0;
    const SplitDev d = make_split_dev(t, false, nt, grid);
    if (t.heads.on && t.heads.small_w) {  // "tower_resident_bf16g+heads": conv policy heads (tower_split_conv_heads_supported)
        if (t.channels == 256) launch<256, 4, false, 2, true>(d, grid, stream);
        else if (nt == 4) launch<128, 4, false, 2, true>(d, grid, stream);
        else if (nt == 7) launch<128, 7, false, 2, true>(d, grid, stream);
        else if (nt == 8) launch<128, 8, false, 2, true>(d, grid, stream);
        else if (nt == 11) launch<128, 11, false, 2, true>(d, grid, stream);
        else if (nt == 13) launch<128, 13, false, 2, true>(d, grid, stream);
        else if (nt == 16) launch<128, 16, false, 2, true>(d, grid, stream);
        else launch<128, 6, false, 2, true>(d, grid, stream);
        return;
    }
    if (t.channels == 512) launch<512, 4, false, 0, true>(d, grid, stream);
    else if (t.channels == 384) launch<384, 4, false, 0, true>(d, grid, stream);
    else if (t.channels == 320 && nt == 6) launch<320, 6, false, 0, true>(d, grid, stream);
    else if (t.channels == 320) launch<320, 4, false, 0, true>(d, grid, stream);
    else if (t.channels == 256 && nt == 6) launch<256, 6, false, 0, true>(d, grid, stream);
    else if (t.channels == 256) launch<256, 4, false, 0, true>(d, grid, stream);
    else if (t.channels == 192 && nt == 4) launch<192, 4, false, 0, true>(d, grid, stream);
    else if (t.channels == 192 && nt == 7) launch<192, 7, false, 0, true>(d, grid, stream);
    else if (t.channels == 192 && nt == 11) launch<192, 11, false, 0, true>(d, grid, stream);
    else if (t.channels == 192 && nt == 8) launch<192, 8, false, 0, true>(d, grid, stream);
    else if (t.channels == 192 && nt == 10) launch<192, 10, false, 0, true>(d, grid, stream);
    else if (t.channels == 192) launch<192, 6, false, 0, true>(d, grid, stream);
    else if (t.channels == 128 && nt == 4) launch<128, 4, false, 0, true>(d, grid, stream);
    else if (t.channels == 128 && nt == 7) launch<128, 7, false, 0, true>(d, grid, stream);
    else if (t.channels == 128 && nt == 8) launch<128, 8, false, 0, true>(d, grid, stream);
    else if (t.channels == 128 && nt == 11) launch<128, 11, false, 0, true>(d, grid, stream);
    else if (t.channels == 128 && nt == 13) launch<128, 13, false, 0, true>(d, grid, stream);
    else if (t.channels == 128 && nt == 16) launch<128, 16, false, 0, true>(d, grid, stream);
    else if (t.channels == 128) launch<128, 6, false, 0, true>(d, grid, stream);
    else if (nt == 4) launch<64, 4, false, 0, true>(d, grid, stream);
    else if (nt == 7) launch<64, 7, false, 0, true>(d, grid, stream);
    else launch<64, 6, false, 0, true>(d, grid, stream);
}

}  // namespace kz
