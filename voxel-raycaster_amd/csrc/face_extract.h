// Kernel-argument block of the face extraction (vrc_extract_faces / vrc_extract_faces_device, include/vrc.h), shared by the host
// layer (vrc_query.cpp) and face_extract.hip.  The scene is a SceneView (vrc_params.h), as in ReadParams (voxel_read.h); the
// regions, their bricks and the numbering of the waves are the region read's.
#pragma once

#include <stdint.h>

#include "vrc_params.h"

namespace vrc {

constexpr int kFaceThreads = 256;                     // 4 waves: the unit of work is one wave per (region, brick)
constexpr int kFaceBrickLog2 = 3;                     // a brick: one map-aligned 8^3 cube, as in voxel_read.h
constexpr uint32_t kFacesNoMapEdge = 1u, kFacesStoppingOnly = 2u;      // VRC_FACES_*

struct FaceParams {
    const int32_t *lo;                // int32[3 n] lower corners
    int64_t n;
    int32_t size[3];                  // the common size (sx, sy, sz), each >= 1
    int64_t bricks[3];                // bricks a region can touch per axis, (size + 6) / 8 + 1
    uint32_t flags;
    int64_t capacity;                 // entries `faces` holds
    int64_t *item_count;              // scratch, one per (region, brick): the faces the brick owns ...
    int64_t *item_end;                // ... and their inclusive scan
    int64_t *counts;                  // int64[n]
    int32_t *faces;                   // int32[4 capacity]: x, y, z, d | material << 8
    SceneView scene;
};

}  // namespace vrc
