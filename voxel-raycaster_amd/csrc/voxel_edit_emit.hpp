// voxel_edit_emit.hpp -- what every brick pass of an edit ends with, once: voxel_edit.hip (single voxels) and region_write.hip
// (boxes and dense blocks) differ in how a wave applies its run to the brick and share how the brick becomes a subtree.  Device
// code only; the Morton helpers live in morton3.hpp, which compiles for the host too.
#pragma once

#include <hip/hip_runtime.h>

#include <stdint.h>

#include "morton3.hpp"
#include "svo_node.hpp"
#include "voxel_edit.h"

namespace vrc {

// first index in [0, n) whose key is not below `key`
__device__ inline int64_t lower_bound(const uint64_t *keys, int64_t n, uint64_t key) {
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (keys[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__device__ inline uint64_t leaf_bits_for(unsigned valid, unsigned leaves) { return (uint64_t)((~valid & 0xffu) | leaves); }

// Row (ly, lz) of the OLD brick with key `key`, as the region read resolves it (svo_node.hpp's node_row); a tree no deeper than a
// brick is read from its root.
__device__ inline uint64_t edit_old_row(const EditParams &q, uint64_t key, int ly, int lz) {
    const int ox = (int)(compact3(key) << kReadBrickLog2), oy = (int)(compact3(key >> 1) << kReadBrickLog2), oz = (int)(compact3(key >> 2) << kReadBrickLog2);
    const int n = q.scene.log2_dim;
    uint64_t old_row = 0;
    if (n >= kReadBrickLog2) {
        uint64_t cur = 0, index = 0;
        const int state = descend_to_node(q.scene, ox, oy, oz, kReadBrickLog2, cur, index);
        if (state == 1) old_row = 0x0505050505050505ULL;
        if (state == 2) old_row = node_row<3>(q.scene, cur, index, ly, lz);
    } else if (ly < (1 << n) && lz < (1 << n)) {
        const uint64_t cur = node_entry(q.scene.descriptors, q.scene.root_index, q.scene.descriptors[VRC_IDX(kDescriptors, q.scene.root_index)]);
        old_row = n == 2 ? node_row<2>(q.scene, cur, q.scene.root_index, ly, lz) : node_row<1>(q.scene, cur, q.scene.root_index, ly, lz);
    }
    return old_row;
}

// The end of a brick pass.  The wave of brick u holds the NEW brick in LDS (rows: 64 words, row (y, z) = lane, byte x; every lane
// of the wave has stored its row and the block has met at a barrier since) and each lane its OLD row.  Counts the voxels that
// differ, builds the brick's subtree -- lane j owns the 2^3 block j = (4^3 child) << 3 | (2^3 child), one ballot gives every mask
// and every rank -- and stores it at brick_base + 72 u, packed, with one attachment word per bottom-level descriptor; leaves the
// brick's record for its parent.  shallow: the tree's depth when the brick holds the whole map (log2_dim <= 3) and the wave emits
// the root itself, else 0.  A wave that is not live takes part in the ballot and stores nothing.
__device__ inline void edit_emit_brick(const EditParams &q, const int shallow, const int64_t u, const int lane, const bool live,
                                       const uint64_t old_row, const uint64_t *rows) {
    const int8_t *bytes = reinterpret_cast<const int8_t *>(rows);
    // voxels whose material differs after the batch
    {
        const uint64_t diff = old_row ^ rows[lane];
        int changed = 0;
        for (int k = 0; k < 8; k++) changed += ((diff >> (8 * k)) & 0xffULL) ? 1 : 0;
        for (int d = 32; d >= 1; d >>= 1) changed += __shfl_down(changed, d, 64);
        if (lane == 0 && changed) atomicAdd(&q.counters[kEditChanged], (unsigned long long)changed);
    }
    // the subtree: lane j owns the 2^3 block `lo` of the 4^3 child `hi`
    const int hi = lane >> 3, lo = lane & 7;
    const int x2 = ((hi & 1) << 1) | (lo & 1), y2 = (((hi >> 1) & 1) << 1) | ((lo >> 1) & 1), z2 = (((hi >> 2) & 1) << 1) | ((lo >> 2) & 1);
    uint64_t mats = 0;
    unsigned valid = 0;
    for (int s = 0; s < 8; s++) {
        const uint8_t b = (uint8_t)bytes[(2 * x2 + (s & 1)) + 8 * ((2 * y2 + ((s >> 1) & 1)) + 8 * (2 * z2 + (s >> 2)))];
        mats |= (uint64_t)b << (8 * s);
        if (b) valid |= 1u << s;
    }
    const uint64_t filled = __ballot(live && valid != 0);         // bit j: block j holds a voxel
    if (!live) return;
    unsigned brick_valid = 0;
    for (int k = 0; k < 8; k++)
        if ((filled >> (8 * k)) & 0xffULL) brick_valid |= 1u << k;
    const uint64_t base = q.brick_base + kEditBrickStride * (uint64_t)u;
    const unsigned n_mid = shallow == 1 ? 0u : (unsigned)__builtin_popcount(brick_valid);
    const uint64_t below_me = (uint64_t)__builtin_popcountll(filled & ((1ULL << lane) - 1ULL));
    if (valid) {
        const uint64_t at = base + n_mid + below_me;
        q.descriptors[at] = ((uint64_t)valid << 16) | kLeafAll;
        if (q.attach_lookup) {
            const uint64_t slot = q.attach_base + kEditBrickAttach * (uint64_t)u + below_me;
            q.attachments[slot] = mats;
            q.attach_lookup[at] = (uint32_t)slot;
        }
    }
    const unsigned mid_valid = (unsigned)(filled >> (8 * hi)) & 0xffu;
    if (lo == 0 && mid_valid && shallow != 1) {
        const uint64_t at = base + (uint64_t)__builtin_popcount(brick_valid & ((1u << hi) - 1u));
        q.descriptors[at] = (base + n_mid + below_me - at) | ((uint64_t)mid_valid << 16) | (leaf_bits_for(mid_valid, 0) << 24);
    }
    if (lane == 0) {
        q.rec_masks[u] = brick_valid | ((uint32_t)leaf_bits_for(brick_valid, 0) << 8);
        q.rec_child[u] = base;
        // a tree no deeper than a brick: the root is the brick's own word (depth 3, in front of the subtree), its 4^3 child 0
        // (depth 2) or its 2^3 block 0 (depth 1), which the lanes above have stored at `base` unless it is empty
        if (shallow == 3) q.descriptors[base - 1] = 1ULL | ((uint64_t)brick_valid << 16) | (leaf_bits_for(brick_valid, 0) << 24);
        if ((shallow == 2 || shallow == 1) && !filled) q.descriptors[base] = kLeafAll;
    }
}

}  // namespace vrc
