// ansfm_merge32_launch.h -- host interface of the 32-bit-key merge kernel's translation unit (ansfm_merge32.hip).
#pragma once
#include <hip/hip_runtime.h>

namespace ansfm {
struct OverlapParams;
// dynamic LDS of one 64-lane block at G g-ordinates
unsigned overlap32_lds_bytes(int G, bool delg_f32);
// p.scratch: [grid][G][64] doubles; the instantiation: the list length of p.G (by_list_len), from_k, p.delg_f32
hipError_t launch_overlap32(const OverlapParams &p, bool from_k, unsigned grid, hipStream_t stream);
}  // namespace ansfm
