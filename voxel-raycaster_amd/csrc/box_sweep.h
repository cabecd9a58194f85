// Kernel-argument block of the batched swept-box queries (vrc_sweep_boxes / vrc_sweep_boxes_device, include/vrc.h), shared by
// the host layer (vrc_query.cpp) and box_sweep.hip.  The scene, the sweeps and the start test's results are a BoxParams: the
// start boxes go through the box query's own passes (box_query.hip, box_stride 9, a list of one voxel) before the sweep kernels run.
#pragma once

#include <stdint.h>

#include "box_query.h"

namespace vrc {

constexpr int kSweepThreads = 256;
// record field 0 (VRC_SWEEP_*)
constexpr int32_t kSweepHit = 1, kSweepStartSolid = 2, kSweepClipped = 4, kSweepRejected = 8, kSweepEventCap = 16, kSweepLeftMap = 32;
// A sweep is one lane while the face of every moving axis (the start range of the other two axes, one layer more each, inside
// the map) holds at most this many voxels, one wave above it (setting sweep_lane_face overrides it; both shapes give the same
// records).  Measured on the MI355X, depth-12 shell terrain, cubes of f voxels, 65 536 sweeps per batch, every sweep forced
// into one shape (profiles/sweep_queries.txt): f = 1 (faces <= 9) lane 0.80 ms, wave 0.86; f = 2 (faces 9 .. 16) lane 1.05,
// wave 0.92; f = 4 lane 2.60, wave 2.16; f = 8 lane 3.62, wave 2.50; f = 32 lane 8.43, wave 5.85.  The crossover lies between
// f = 1 and f = 2; 12 keeps player-sized boxes (0.6 x 0.6 x 1.8: faces <= 3 x 4), whose batches are the large ones, as lanes.
// Not measured: the same comparison at 1 M sweeps per batch, where a wave per sweep means 16 times as many waves.
constexpr int32_t kSweepLaneFaceMax = 12;

struct SweepParams {
    BoxParams box;                    // boxes: float[9 * n] origin, extent, displacement (box_stride 9); flags: kBoxStoppingOnly;
                                      // records / voxels: the start test's output (max_voxels 1); the scene
    int32_t *records;                 // int32[8 * n]
    int32_t cap;                      // events per sweep (bounds the loop)
    int32_t lane_face_max;
    const int64_t *big_end;           // [n] inclusive scan of "this sweep is a wave": wave k's sweep is the first with big_end > k
    int64_t n_big;
};

}  // namespace vrc
