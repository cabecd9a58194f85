// Kernel-argument blocks of the voxel edits (vrc_set_voxels / vrc_set_voxels_device, include/vrc.h), shared by the host layer
// (vrc_scene_edit.cpp) and voxel_edit.hip.  The scene is a SceneView (vrc_params.h) of the tree BEFORE the edit; the edit reads only
// words below its n_desc and stores only at and above it.
#pragma once

#include <stdint.h>

#include "voxel_read.h"
#include "vrc_params.h"

namespace vrc {

constexpr int kEditThreads = 256;                     // 4 waves: the brick pass's unit of work is one wave
constexpr int kEditBrickVoxels = 1 << (3 * kReadBrickLog2);
// the words a touched brick / a touched node above the bricks owns in the appended range, whatever it stores there (the rest
// stays zero): 8 descriptors of 4^3 nodes + 64 bottom-level descriptors; 8 child descriptors + their 8 far slots
constexpr uint64_t kEditBrickStride = 72, kEditNodeStride = 16;
constexpr uint64_t kEditBrickAttach = 64;             // attachment slots per touched brick: one per bottom-level descriptor
enum EditCounter { kEditSkipped = 0, kEditChanged, kEditMaterials, kEditRuns, kEditCounters };

struct EditParams {
    const int32_t *positions;         // int32[3 n]
    const int32_t *materials;         // int32[n]
    int64_t n;
    uint64_t sentinel;                // the key of a skipped edit: above every key of the scene
    uint64_t *keys; uint32_t *order;  // key pass out: the brick's Morton key (array branch: the voxel's index), the edit number
    const uint64_t *sorted_keys; const uint32_t *sorted_order;    // ... sorted by (key, edit number)
    unsigned long long *counters;     // EditCounter
    int8_t *map;                      // array branch: the map the scatter stores into
    // brick pass: the touched bricks in key order, where their subtrees and attachment slots go, what they leave for their parents
    const uint64_t *brick_keys; int64_t n_bricks;
    uint64_t *descriptors; uint32_t *attach_lookup; uint64_t *attachments;    // the arrays the edit appends to (materials optional)
    uint64_t brick_base, attach_base;
    uint32_t *rec_masks; uint64_t *rec_child;         // per touched node: valid | leaf << 8 (valid 0: empty), index of its child block
    SceneView scene;
};

// One launch of the ancestor pass: the touched nodes of size 2^r (keys: the unique key >> 3 of the level below), their
// records at rec_here, the level below's keys and records.  root: the level is the root's; the new root word goes to `base` and
// the root's child block follows it.
struct EditLevel {
    const uint64_t *keys; int64_t count;
    const uint64_t *below_keys; int64_t below_count;
    int64_t rec_here, rec_below;
    uint64_t base;
    int32_t r, root;
};

}  // namespace vrc
