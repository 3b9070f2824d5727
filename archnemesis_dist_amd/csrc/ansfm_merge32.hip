// ansfm_merge32.hip -- translation unit of k_ck_overlap32 (ansfm_merge32.hip.h): the instantiations and their launcher.
#include "ansfm_merge32.hip.h"
#include "ansfm_merge32_launch.h"

namespace ansfm {

unsigned overlap32_lds_bytes(int G, bool delg_f32) { return m32_lds_bytes(G, delg_f32); }

hipError_t launch_overlap32(const OverlapParams &p, bool from_k, unsigned grid, hipStream_t stream)
{
    const size_t lds = m32_lds_bytes(p.G, p.delg_f32 != 0);
    using Kernel32 = void (*)(OverlapParams);
    const bool w32 = p.delg_f32 != 0;
    const Kernel32 kern = by_list_len(p.G, [&](auto d) -> Kernel32 {
        constexpr int D = decltype(d)::value;
        if (from_k) return w32 ? k_ck_overlap32<D, true, true> : k_ck_overlap32<D, true, false>;
        return w32 ? k_ck_overlap32<D, false, true> : k_ck_overlap32<D, false, false>;
    });
    hipLaunchKernelGGL(kern, dim3(grid), dim3(kWave), lds, stream, p);
    return hipGetLastError();
}

}  // namespace ansfm
