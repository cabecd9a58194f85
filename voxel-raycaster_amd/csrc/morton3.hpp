// morton3.hpp -- the two bit tricks behind every brick key of the scene edits (voxel_edit.hip, region_write.hip,
// voxel_edit_emit.hpp): a brick's key is spread3(bx) | spread3(by) << 1 | spread3(bz) << 2.  A header of their own because they
// compile for the host as they stand, so tests/morton3_check.cpp checks them on the CPU against a loop over single bits.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define VRC_MORTON_FN __host__ __device__ inline
#else
#define VRC_MORTON_FN inline
#endif

namespace vrc {

// bit k of v to bit 3 k (21 bits), and back
VRC_MORTON_FN uint64_t spread3(uint64_t x) {
    x &= 0x1fffffULL;
    x = (x | x << 32) & 0x1f00000000ffffULL;
    x = (x | x << 16) & 0x1f0000ff0000ffULL;
    x = (x | x << 8) & 0x100f00f00f00f00fULL;
    x = (x | x << 4) & 0x10c30c30c30c30c3ULL;
    x = (x | x << 2) & 0x1249249249249249ULL;
    return x;
}
VRC_MORTON_FN uint32_t compact3(uint64_t x) {
    x &= 0x1249249249249249ULL;
    x = (x ^ (x >> 2)) & 0x10c30c30c30c30c3ULL;
    x = (x ^ (x >> 4)) & 0x100f00f00f00f00fULL;
    x = (x ^ (x >> 8)) & 0x1f0000ff0000ffULL;
    x = (x ^ (x >> 16)) & 0x1f00000000ffffULL;
    x = (x ^ (x >> 32)) & 0x1fffffULL;
    return (uint32_t)x;
}

}  // namespace vrc
