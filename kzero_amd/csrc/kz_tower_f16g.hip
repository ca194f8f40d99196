// kz_tower_f16g.hip — the SPLIT = false instances of kz_tower_pairs.hpp: the same one-launch tower in plain f16 (one image per
// activation, one MFMA per product, f16 tensors in and out) for the shapes kz_tower.hip (chess: 8x8, 256 channels, attention
// heads) does not take — KZ_DTYPE_F16's "tower_resident_f16g[+heads]": 64 .. 512 channels on small boards, with the wide tiles
// (twice the boards per workgroup) at 128 / 192 channels.  The kernel's body is in kz_tower_pairs.hpp; which instances exist
// is the table PLAIN_ROWS in kz_tower_pairs_shapes.hpp, and launch_pairs compiles exactly those here (BF = false) and
// launches the one a shape's tiles name.
#include "kz_tower_pairs.hpp"

namespace kz {

bool launch_tower_pairs(const Tower32Args &t, hipStream_t stream, int *nt) { return launch_pairs<false, false>(t, stream, nt); }

}  // namespace kz
