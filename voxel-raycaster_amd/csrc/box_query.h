// Kernel-argument block of the batched box-overlap queries (vrc_box_intersection / vrc_box_intersection_device,
// include/vrc.h), shared by the host layer (vrc_query.cpp) and box_query.hip.  The scene is a SceneView (vrc_params.h), as in
// QueryParams (raycast_query.h); the scratch pointers are the host layer's, sized from what the plan pass reports.  Nothing
// of a frame's buffers is in here.
#pragma once

#include <stdint.h>

#include "vrc_params.h"

namespace vrc {

constexpr int kBoxThreads = 256;
constexpr uint32_t kBoxStoppingOnly = 1u;             // VRC_BOX_STOPPING_ONLY
// record field 0 (VRC_BOX_*)
constexpr int32_t kBoxAny = 1, kBoxTruncated = 2, kBoxClipped = 4, kBoxRejected = 8;
// items: aligned nodes of 2^s voxels, 2 <= 2^s; a box's nodes are at most 64 per axis span (so <= 65^3 items per box)
constexpr int kBoxMaxItemLog2 = 6;                    // the node size grows with the box up to 64 ...
constexpr int kBoxItemsPerAxisLog2 = 6;               // ... and beyond that only as far as 64 nodes per axis need
constexpr int kBoxSmallItemLog2 = 2;                  // items of <= 4^3 voxels are one lane; larger ones a wave of 64 lanes

// per-box plan (box_plan_kernel): the clipped range, the item size and where the box's items sit in their item space
struct BoxPlan {
    int32_t lo[3], hi[3];             // clipped voxel range [lo, hi) per axis; lo == hi on some axis: nothing to examine
    int32_t s_log2;                   // item node size 2^s_log2
    int32_t kind;                     // 0 no items, 1 lane items (small space), 2 wave items (big space)
    int32_t flags;                    // kBoxClipped / kBoxRejected
};

struct BoxParams {
    const float *boxes;               // float[box_stride * n]: origin xyz, extent xyz (then what a sweep adds: box_sweep.h)
    int32_t box_stride;               // 6 for a box query
    int64_t n;
    int32_t max_voxels;
    uint32_t flags;                   // kBoxStoppingOnly
    int32_t *records;                 // int32[8 * n]
    int64_t *counts;                  // int64[n]
    int32_t *voxels;                  // int32[4 * max_voxels * n] (nullptr iff max_voxels == 0)
    SceneView scene;
    int32_t space_log2;               // the aligned space the items tile: 2^log2_dim (tree), the map's largest side rounded up (array)
    // scratch (device)
    BoxPlan *plan;                    // [n]
    int64_t *small_end;               // [n] inclusive scan of the boxes' lane-item counts
    int64_t *big_end;                 // [n] inclusive scan of the boxes' wave-item counts
    int64_t *acc_count;               // [n] per-box totals (atomics: integer sums, order-free)
    int32_t *acc_corner;              // [6 n] per-box min xyz, max xyz (atomic integer min / max, order-free)
    int64_t *item_count;              // [small + big] per-item counts (emit only; small items first)
    int64_t *item_end;                // [small + big] their inclusive scan (emit only)
    int64_t n_small, n_big;           // item totals (from the plan's scans)
};

}  // namespace vrc
