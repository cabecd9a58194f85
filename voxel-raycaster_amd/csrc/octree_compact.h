// Kernel-argument blocks of the octree compaction (vrc_compact_octree, include/vrc.h), shared by the host layer (vrc_scene_edit.cpp)
// and octree_compact.hip.  The scene is a SceneView (vrc_params.h) of the tree BEFORE the call; the passes read only that tree
// and store only into the new arrays and the call's own scratch.
#pragma once

#include <stdint.h>

#include "vrc_params.h"

namespace vrc {

constexpr int kCompactThreads = 256;
constexpr int64_t kCompactReachMin = 16, kCompactReachMax = 0x7fff;       // setting compact_near_reach
// kCompactFar: far slots of the new array; kCompactBad: indices outside an array that a pass met (the old tree is corrupt, or a
// placement left the new array: the access is not made and the call fails)
enum CompactCounter { kCompactFar = 0, kCompactBad, kCompactCounters };

struct CompactParams {
    SceneView scene;                  // the old tree (no coarse table: nothing here descends by position)
    uint64_t n_old, n_attach_old;     // its extents
    uint64_t reach;
    uint64_t *out; uint64_t n_out;    // the new array and its words (emit only; nullptr: a dry run, which stores nothing)
    uint32_t *out_lookup;             // the new lookup, zeroed by the host (nullptr: a tree without materials, a dry run)
    uint64_t *used;                   // per old attachment slot: 1 when a reachable bottom-level descriptor names it (nullptr: no materials)
    unsigned long long *counters;     // CompactCounter
};

// One level's list: the descriptors of level `level` that hold a pointer, by old index, in the order of the new array.  An
// entry's pointer-holding children are the entries scan[i] + rank of the level below.
struct CompactLevel {
    const uint64_t *list; int64_t count;
    int32_t level, children_bottom;   // children_bottom: the children are bottom-level descriptors and enter no list
    uint8_t *pmask, *farmask;         // per entry, a bit per child slot: the child holds a pointer; its pointer is far
    uint64_t *cnt;                    // gather: count + 1 words, popcount(pmask) and a zero at the end, for the scan
    const uint64_t *scan;             // its exclusive scan (scan[count]: the entries of the level below)
    uint64_t *next_list;
    uint64_t *size; const uint64_t *size_below;       // S: the words of an entry's subtree without its own
    const uint64_t *base; uint64_t *base_below;       // B: where an entry's child block starts in the new array
};

}  // namespace vrc
