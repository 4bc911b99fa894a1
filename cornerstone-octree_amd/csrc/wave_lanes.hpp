// Cross-lane partners of a wave on the VALU (no LDS pipe): DPP within a row of 16 lanes, v_permlane16/32_swap (gfx950)
// across rows; lane mappings verified with tools/dpp_probe.hip on the hardware.  Shared by the register-resident sorting
// networks of resort.hip (32-bit digests) and knn.hip (distance keys of two or three words).
#pragma once

#include <cstdint>

#include <hip/hip_runtime.h>

namespace cship
{

template<int CTRL, int BANK>
__device__ __forceinline__ uint32_t dppMov(uint32_t old, uint32_t v)
{
    return uint32_t(__builtin_amdgcn_update_dpp(int(old), int(v), CTRL, 0xF, BANK, false));
}
//! a permutation inside the row in which every lane has a source: written so that the compiler may fold it into the
//! operation that consumes it (v_min_u32_dpp / v_max_u32_dpp)
template<int CTRL>
__device__ __forceinline__ uint32_t dppAll(uint32_t v)
{
    return uint32_t(__builtin_amdgcn_update_dpp(0, int(v), CTRL, 0xF, 0xF, true));
}
//! value of lane ^ X
template<int X>
__device__ __forceinline__ uint32_t laneXor(uint32_t v, unsigned lane)
{
    if constexpr (X == 1) return dppAll<0xB1>(v);        // quad_perm [1,0,3,2]
    else if constexpr (X == 2) return dppAll<0x4E>(v);   // quad_perm [2,3,0,1]
    else if constexpr (X == 3) return dppAll<0x1B>(v);   // quad_perm [3,2,1,0]
    else if constexpr (X == 7) return dppAll<0x141>(v);  // row_half_mirror
    else if constexpr (X == 15) return dppAll<0x140>(v); // row_mirror
    else if constexpr (X == 4)
    {
        const uint32_t t = dppMov<0x104, 0x5>(v, v); // row_shl:4 into banks 0 and 2 (lane reads lane + 4)
        return dppMov<0x114, 0xA>(t, v);             // row_shr:4 into banks 1 and 3 (lane reads lane - 4)
    }
    else if constexpr (X == 8)
    {
        const uint32_t t = dppMov<0x108, 0x3>(v, v);
        return dppMov<0x118, 0xC>(t, v);
    }
    else if constexpr (X == 16)
    {
        auto p = __builtin_amdgcn_permlane16_swap(v, v, false, false); // [0]: rows 0,0,2,2   [1]: rows 1,1,3,3
        return (lane & 16u) ? p[0] : p[1];
    }
    else if constexpr (X == 32)
    {
        auto p = __builtin_amdgcn_permlane32_swap(v, v, false, false); // [0]: lower half twice   [1]: upper half twice
        return (lane & 32u) ? p[0] : p[1];
    }
    else if constexpr (X == 31) return laneXor<15>(laneXor<16>(v, lane), lane);
    else
    {
        static_assert(X == 63, "partner not implemented");
        return laneXor<15>(laneXor<16>(laneXor<32>(v, lane), lane), lane);
    }
}

} // namespace cship
