// Kernel-argument block of the voxel reads (vrc_get_voxels / vrc_read_regions and their _device variants, include/vrc.h),
// shared by the host layer (vrc_api.cpp) and voxel_read.hip.  The scene fields are those of BoxParams (box_query.h) under the
// same names, so the host layer binds them the same way.  There is no scratch: a read is one launch.
#pragma once

#include <stdint.h>

namespace vrc {

constexpr int kReadThreads = 256;                     // 4 waves: a region read's unit of work is one wave
constexpr int kReadBrickLog2 = 3;                     // a brick: one map-aligned 8^3 cube, one level-3 node, 64 rows of 8 voxels

struct ReadParams {
    const int32_t *positions;         // points: int32[3 n] voxel positions; regions: int32[3 n] lower corners
    int64_t n;
    int32_t *values;                  // points: int32[n]
    int8_t *bytes;                    // regions: int8[n * size[0] * size[1] * size[2]], any alignment
    int32_t size[3];                  // regions: the common size (sx, sy, sz), each >= 1
    int64_t bricks[3];                // regions: bricks a region can touch per axis, (size + 6) / 8 + 1
    // scene (the branch and the tree as in BoxParams)
    int32_t svo;
    const int8_t *map;                // array branch
    int32_t map_dim[3];
    uint64_t map_bytes;
    const uint64_t *descriptors;
    uint64_t root_index;
    int32_t log2_dim;
    const uint32_t *attach_lookup;
    const uint64_t *attachments;
    const uint64_t *coarse;           // nullptr: descend from the root
    int32_t coarse_log2;
};

}  // namespace vrc
