// Kernel-argument block of the voxel reads (vrc_get_voxels / vrc_read_regions and their _device variants, include/vrc.h),
// shared by the host layer (vrc_query.cpp) and voxel_read.hip.  The scene is a SceneView (vrc_params.h), as in BoxParams
// (box_query.h).  There is no scratch: a read is one launch.
#pragma once

#include <stdint.h>

#include "vrc_params.h"

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
    SceneView scene;
};

}  // namespace vrc
