// Kernel-argument block of the batched ray queries (vrc_cast_rays / vrc_cast_rays_device, include/vrc.h), shared by the
// host layer (vrc_api.cpp) and raycast_query.hip.  The scene fields are those of RaycastParams (vrc_params.h) that a query
// reads; nothing of a frame's buffers (image, hit records, counters, the frame constants) is in here, so a query cannot
// disturb what a frame reports.
#pragma once

#include <stdint.h>

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
    int32_t svo;                      // using_octree == 0: the tree; else the dense char map
    int32_t octree_bias;              // setting octree_bias (AS_PIXEL only)
    const int8_t *map;                // array branch
    int32_t map_dim[3];
    uint64_t map_bytes;
    const uint64_t *descriptors;      // the tree (both branches: the AS_PIXEL bias reads it, as frame_setup_kernel does)
    uint64_t root_index;
    int32_t log2_dim;
    const uint32_t *attach_lookup;    // materials (optional, SVO branch)
    const uint64_t *attachments;
    const uint64_t *coarse;           // the tree's top as a dense table (nullptr: descend from the root)
    int32_t coarse_log2;
    const uint32_t *boxes;            // empty boxes (nullptr: none; needs the table)
    const uint32_t *box_aux;
    const uint32_t *box_child;        // box records for the upper levels only (nullptr: a word per descriptor)
    int32_t box_levels;
};

}  // namespace vrc
