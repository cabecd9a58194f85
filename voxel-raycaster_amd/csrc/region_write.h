// Kernel-argument block of the region edits (vrc_fill_boxes / vrc_write_regions / vrc_fill_shapes and their _device variants, include/vrc.h),
// shared by the host layer (vrc_scene_edit.cpp) and region_write.hip.  The front end turns the operations into (brick key, operation)
// pairs; from the sorted pairs on the edit's own argument block (voxel_edit.h) carries everything, so `edit` is filled the way
// vrc_set_voxels fills it: sorted_keys / sorted_order / n are the pairs, brick_keys / n_bricks the touched bricks.
#pragma once

#include <stdint.h>

#include "voxel_edit.h"

namespace vrc {

// vrc.h's VRC_WRITE_* bits
constexpr uint32_t kWriteWhereEmpty = 1u, kWriteWhereSolid = 2u, kWriteSkipZero = 4u;

constexpr int32_t kRegionFill = 0, kRegionPaste = 1, kRegionShapes = 2;

struct RegionParams {
    // the operations.  Fill: boxes int32[6 n] = lo, size; materials int32[n].  Paste: boxes int32[3 n] = lo, the common size in
    // `size`, data = n blocks of `volume` bytes.  Shapes: boxes int32[6 n] = kind, centre, r, h (shape_span.hpp's ShapeOp);
    // materials int32[n].
    const int32_t *boxes;
    const int32_t *materials;
    const int8_t *data;
    int64_t n;
    int32_t size[3];
    int32_t mode;                     // kRegionFill, kRegionPaste or kRegionShapes (the fills' brick pass with a span per row)
    uint32_t flags;
    int32_t scan_materials;           // paste: look at the bytes for a material other than 0 and 5 (a tree without attachments)
    uint64_t volume;
    // the scene the operations are clipped to and its bricks per axis.  Tree: [0, dim)^3, keys are Morton keys.  Map: map_dim with
    // z cut where the frame's index leaves the array; keys are bx + nb[0] * (by + nb[1] * bz).
    int32_t lim[3];
    int64_t nb[3];
    uint64_t *counts, *offsets;       // [n + 1]: bricks per operation (counts[n] = 0), their exclusive scan (offsets[n]: the pairs)
    EditParams edit;
};

}  // namespace vrc
