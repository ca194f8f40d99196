// kz_tower_split.hip — the SPLIT = true instances of kz_tower_pairs.hpp: the board-resident ResTower with f32-EQUIVALENT results
// on the f16 matrix cores (every activation and weight a (hi, lo) f16 pair, three MFMAs per product, f32 accumulation),
// KZ_DTYPE_F32_SPLIT16's "tower_resident_split16[+heads]".  The kernel's body, its LDS geometry and the arithmetic are in
// kz_tower_pairs.hpp; which instances exist is the table SPLIT_ROWS (and SPLIT_ATTENTION, the chess attention network) in
// kz_tower_pairs_shapes.hpp, and launch_pairs compiles exactly those here and launches the one a shape's tiles name.
// (Python: python/lib/model/post_act.py:201-239; the fused heads :10-23, :54-141.)
#include "kz_tower_pairs.hpp"

namespace kz {

bool launch_tower_split(const Tower32Args &t, hipStream_t stream, int *nt) { return launch_pairs<true>(t, stream, nt); }

}  // namespace kz
