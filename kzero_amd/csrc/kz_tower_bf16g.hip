// kz_tower_bf16g.hip — the BF = true instances of kz_tower_pairs.hpp: the one-launch tower of kz_tower_f16g.hip with bf16 as the
// element of its images, weight fragments and MFMAs (v_mfma_f32_16x16x32_bf16, f32 accumulation; bias, ReLU, residual add and
// the final BN in f32) and f32 tensors at its boundary — dtype 3's "tower_resident_bf16g[+heads]": f32's range at the f16
// rate, 8 significant bits.  Same shapes, tiles and choice among them as the plain-f16 family (64 .. 512 channels on small
// boards, the wide tiles at 128 / 192 channels): the same table, PLAIN_ROWS in kz_tower_pairs_shapes.hpp, and the same call
// with BF = true; the conv heads' tail inside the launch is exact f32.  The kernel's body is in kz_tower_pairs.hpp.
#include "kz_tower_pairs.hpp"

namespace kz {

bool launch_tower_bf16(const Tower32Args &t, hipStream_t stream, int *nt) { return launch_pairs<false, true>(t, stream, nt); }

}  // namespace kz
