// Kernel-argument block of the batched ray queries (vrc_cast_rays / vrc_cast_rays_device, include/vrc.h), shared by the
// host layer (vrc_query.cpp) and raycast_query.hip.  The scene is a SceneView (vrc_params.h), bound by the host layer's
// bind_scene like every query family's; nothing of a frame's buffers (image, hit records, counters, the frame constants) is
// in here, so a query cannot disturb what a frame reports.
#pragma once

#include <stdint.h>

#include "vrc_params.h"

namespace vrc {

constexpr int kQueryThreads = 256;
constexpr uint32_t kQueryAsPixel = 1u;                 // VRC_RAY_AS_PIXEL
// record field 5 (VRC_RAY_*)
constexpr int32_t kRayHit = 1, kRayLeftMap = 2, kRayStepCap = 4, kRayRejected = 8;

struct QueryParams {
    const float *rays;                // float[6 * n]: origin xyz, direction xyz
    int32_t *out;                     // int32[8 * n]
    int64_t n;
    int32_t cap;                      // iterations a ray may take (max_steps, or 3 * dim + 3 for max_steps = 0)
    uint32_t flags;                   // kQueryAsPixel
    int32_t octree_bias;              // setting octree_bias (AS_PIXEL only)
    SceneView scene;                  // (the tree is bound in both branches: the AS_PIXEL bias reads it, as frame_setup_kernel does)
    const uint32_t *boxes;            // empty boxes (nullptr: none; needs the table)
    const uint32_t *box_aux;
    const uint32_t *box_child;        // box records for the upper levels only (nullptr: a word per descriptor)
    int32_t box_levels;
};

}  // namespace vrc
