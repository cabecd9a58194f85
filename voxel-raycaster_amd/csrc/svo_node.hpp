// svo_node.hpp -- the octree descriptor format, once, for every piece of code that reads it: the frame kernels, the query,
// box, sweep and voxel-read kernels, the coarse-table and empty-box builders, the device builder's validators and the host
// builder.  Compiles for the device and the host.  (The oracle and the numpy replays under tests/ restate the format on
// purpose and do not share this file.)  Two places keep copies of their own, because as calls they compile to another
// instruction stream and the frame kernels' code is kept as it was (profiles/r10_descriptor_header.txt): raycast_kernel.hip
// writes out the sibling-widening rule (its widen_word lambda and enter_node; widen_axes below serves raycast_query.hip) and
// frame_setup_kernel writes out get_oct_vox.
//
// A descriptor is one 64-bit word of the array (the reference's child descriptor, include/map/Octree.h):
//   bits 0-14   pointer to the first kept child, relative to the descriptor's own index
//   bit  15     far flag: the slot at that offset holds the absolute index of the first kept child instead
//   bits 16-23  valid mask, one bit per child slot x | y << 1 | z << 2: the child holds something
//   bits 24-31  leaf mask: the valid child is solid throughout and has no descriptor
// The child block counts the valid slots in slot order, so the kept child in slot k sits at
// first + popcount(valid at or below k) - 1.  At the bottom level (the children are voxels) every valid slot is a solid
// voxel whatever the leaf mask says.
//
// The walkers carry a descriptor as a packed ENTRY with the far pointer resolved:
//   bits 0-7 valid mask, 8-15 leaf mask, 16-63 absolute index of the first kept child
// and a cell of the coarse table (vrc_params.h) is such an entry with the level of its node in bits 59-63.
#pragma once

#include <stdint.h>

#include "index_audit.hpp"
#include "vrc_params.h"

// VRC_NODE_FN: the small helpers, always inlined; VRC_NODE_WALK: the descents
#if defined(__HIPCC__)
#define VRC_NODE_WALK __host__ __device__ inline
#else
#define VRC_NODE_WALK inline
#endif
#define VRC_NODE_FN VRC_NODE_WALK __attribute__((always_inline))

namespace vrc {

constexpr uint64_t kNearMask = 0x7fffULL, kFarBit = 0x8000ULL, kValidAll = 0x00FF0000ULL, kLeafAll = 0xFF000000ULL;

// index of the first kept child of the descriptor d at `index`
VRC_NODE_FN uint64_t first_child(const uint64_t *__restrict__ descriptors, uint64_t index, uint64_t d) {
    uint64_t base = index + (d & kNearMask);
    if (d & kFarBit) base = descriptors[VRC_IDX(kFarSlots, base)];            // far pointer: the slot holds an absolute index
    return base;
}

// the packed entry of the descriptor d at `index`
VRC_NODE_FN uint64_t node_entry(const uint64_t *__restrict__ descriptors, uint64_t index, uint64_t d) {
    return (first_child(descriptors, index, d) << 16) | ((d >> 16) & 0xffffULL);   // (leaf << 8 | valid) are bits 16..31 of d
}

// place of child slot `slot` among the kept children (masks: the valid mask in bits 0-7; the slot is valid)
VRC_NODE_FN unsigned child_rank(unsigned masks, unsigned slot) {
    return (unsigned)__builtin_popcount(masks & 0xffu & ((2u << slot) - 1u)) - 1u;
}

// index of the kept child in slot `slot` of the node with entry `entry`
VRC_NODE_FN uint64_t kept_child(uint64_t entry, unsigned slot) { return (entry >> 16) + (uint64_t)child_rank((unsigned)entry, slot); }

// child slot of voxel (x, y, z) in a node whose children are 2^b voxels wide
VRC_NODE_FN int child_slot(int x, int y, int z, int b) { return ((x >> b) & 1) | (((y >> b) & 1) << 1) | (((z >> b) & 1) << 2); }

// a cell of the coarse table: the entry, and the level of its node
VRC_NODE_FN uint64_t coarse_cell_entry(uint64_t e) { return e & ((1ULL << kCoarseLevelShift) - 1ULL); }
VRC_NODE_FN int coarse_cell_level(uint64_t e) { return (int)(e >> kCoarseLevelShift); }
VRC_NODE_FN uint64_t coarse_cell_pack(uint64_t entry, int level) { return entry | ((uint64_t)level << kCoarseLevelShift); }

// The reference's get_oct_vox (kernels/ray_caster_kernel.cl:140-251) / Octree::GetVoxel (src/map/Octree.cpp:45-158) for the
// voxel at `pos` of a tree of `dimension` voxels per axis: the running corner of the node the descent ends in, `resolution`
// (halved per level taken, not at a leaf) and the descriptors read.
struct OctVox { int found, resolution, corner[3], reads; };
VRC_NODE_WALK OctVox get_oct_vox(const uint64_t *descriptors, uint64_t root_index, int dimension, const int pos[3]) {
    OctVox v = {1, dimension / 2, {0, 0, 0}, 1};
    uint64_t index = root_index, d = descriptors[VRC_IDX(kDescriptors, index)];
    while (dimension > 1) {
        const int half = dimension / 2;
        int i = 0;
        for (int a = 0; a < 3; a++)
            if (pos[a] >= v.corner[a] + half) { i |= 1 << a; v.corner[a] += half; }
        if (!((d >> (16 + i)) & 1ULL)) { v.found = 0; break; }    // not valid: empty node
        if ((d >> (24 + i)) & 1ULL) break;                        // valid leaf: early exit, resolution not halved
        dimension = half;
        v.resolution /= 2;
        index = first_child(descriptors, index, d) + (uint64_t)child_rank((unsigned)(d >> 16), (unsigned)i);
        d = descriptors[VRC_IDX(kDescriptors, index)];
        v.reads++;
    }
    return v;
}

// the 8 materials of the bottom-level descriptor at `index` (one byte per child slot; only the valid slots mean something)
VRC_NODE_FN uint64_t bottom_materials(const SceneView &s, uint64_t index) {
    return s.attach_lookup ? s.attachments[VRC_IDX(kAttachments, s.attach_lookup[VRC_IDX(kAttachLookup, index)])] : 0x0505050505050505ULL;
}

// Descend to the node of size 2^r at (cx, cy, cz) inside the map, r >= 0 -- from the coarse table's cell when the table is
// there and the node is no larger than a cell, from the root otherwise: 0 the node is empty, 1 it lies inside a solid leaf,
// 2 it has a descriptor (cur its entry, cur_index its index; r >= 1), 3 it is a single solid voxel of a bottom-level
// descriptor (r == 0: cur and cur_index are its parent's).  A node below the root that is the table cell's own comes without
// its index -- the table does not hold it -- and cur_index is kNoIndex then: the callers need the index of bottom-level
// descriptors only, and a cell's node is never one.
constexpr uint64_t kNoIndex = ~0ULL;
VRC_NODE_WALK int descend_to_node(const SceneView &s, int cx, int cy, int cz, int r, uint64_t &cur, uint64_t &cur_index) {
    const int n = s.log2_dim;
    int top;
    cur_index = s.root_index;
    if (s.coarse && r <= n - s.coarse_log2) {
        const int csh = n - s.coarse_log2;
        const uint64_t e = s.coarse[VRC_IDX(kCoarse, coarse_index((unsigned)(cx >> csh), (unsigned)(cy >> csh), (unsigned)(cz >> csh), s.coarse_log2))];
        cur = coarse_cell_entry(e);
        top = coarse_cell_level(e);
        if (top > 0) cur_index = kNoIndex;
    } else {
        cur = node_entry(s.descriptors, s.root_index, s.descriptors[VRC_IDX(kDescriptors, s.root_index)]);
        top = 0;
    }
    for (int guard = 0; guard <= n && n - top > r; guard++) {             // (n + 1 levels at most: a corrupt tree cannot loop)
        const int b = n - top - 1;
        const int i = child_slot(cx, cy, cz, b);
        const unsigned masks = (unsigned)cur & 0xffffu, bit = 1u << i;
        if (!(masks & bit)) return 0;
        if (b == 0) return 3;
        if ((masks >> 8) & bit) return 1;
        cur_index = kept_child(cur, (unsigned)i);
        cur = node_entry(s.descriptors, cur_index, s.descriptors[VRC_IDX(kDescriptors, cur_index)]);
        top++;
    }
    return 2;
}

// material of voxel (x, y, z) inside the map of the tree: a valid leaf slot at any level or any valid slot at the bottom level
// is solid, with the attachment byte for bottom-level descriptors when attachments are assigned, else 5; 0 is empty
VRC_NODE_WALK int voxel_material(const SceneView &s, int x, int y, int z) {
    uint64_t cur = 0, index = 0;
    const int state = descend_to_node(s, x, y, z, 0, cur, index);
    if (state == 3) return (int)(int8_t)(bottom_materials(s, index) >> (8 * child_slot(x, y, z, 0)));
    return state == 1 ? 5 : 0;
}

// The 2^kLevel voxels along x of row (y, z) of the node `cur` (at `index`, of size 2^kLevel, kLevel <= 3), one byte each, lowest
// x first: the unit of the region read (voxel_read.hip) and of the edit's brick pass (voxel_edit.hip), a lane per row.
template <int kLevel>
VRC_NODE_FN uint64_t node_row(const SceneView &s, uint64_t cur, uint64_t index, int y, int z) {
    constexpr int cb = kLevel - 1;                        // the children are 2^cb voxels wide
    const int yz = (((y >> cb) & 1) << 1) | (((z >> cb) & 1) << 2);
    const unsigned masks = (unsigned)cur & 0xffffu;
    uint64_t row = 0;
    if constexpr (kLevel == 1) {
        if (masks & (3u << yz)) {
            const uint64_t mats = bottom_materials(s, index);
            for (int h = 0; h < 2; h++)
                if (masks & (1u << (yz | h))) row |= ((mats >> (8 * (yz | h))) & 0xffULL) << (8 * h);
        }
    } else {
        constexpr uint64_t solid = 0x0505050505050505ULL >> (64 - 8 * (1 << cb));       // 2^cb bytes of 5
        for (int h = 0; h < 2; h++) {
            const unsigned bit = 1u << (yz | h);
            uint64_t half = 0;
            if (masks & bit) {
                if ((masks >> 8) & bit) {
                    half = solid;
                } else {
                    const uint64_t child = kept_child(cur, (unsigned)(yz | h));
                    half = node_row<kLevel - 1>(s, node_entry(s.descriptors, child, s.descriptors[VRC_IDX(kDescriptors, child)]), child, y, z);
                }
            }
            row |= half << (8 * h * (1 << cb));
        }
    }
    return row;
}

// An empty-box word (empty_boxes.hip) holds six 5-bit extent codes, in units of the node's size: the extent of code c
VRC_NODE_FN int box_extent(unsigned c) { return c < 4u ? (int)c : (int)((4u | (c & 3u)) << ((c >> 2) - 1u)); }

// The sibling-widening rule: the axes over which the empty child `slot` of a node with valid mask `valid` can be doubled, given
// the axes `ahead` on which the ray moves from this half of the parent toward the other half.  All of them when every sibling
// they cover is empty, else one axis, y before x before z (the children covered when widening over the axes in e are those that
// differ from the slot only in axes of e: the subsets of e as bit positions, one byte per e in the constant, shifted to the
// slot with the axes of e cleared).
VRC_NODE_FN unsigned widen_axes(unsigned valid, unsigned slot, unsigned ahead) {
    auto span = [&](unsigned e) -> unsigned { return ((unsigned)(0xFF5533110F050301ULL >> (8u * e)) & 0xffu) << (slot & ~e); };
    auto pair = [&](unsigned e) -> unsigned { return (1u << slot) | (1u << (slot ^ e)); };   // span of one axis
    unsigned ext = 0;
    if ((span(ahead) & valid) == 0) ext = ahead;
    else if ((ahead & 2u) && (pair(2u) & valid) == 0) ext = 2u;
    else if ((ahead & 1u) && (pair(1u) & valid) == 0) ext = 1u;
    else if ((ahead & 4u) && (pair(4u) & valid) == 0) ext = 4u;
    return ext;
}
// ... and the result as a box word: extent code 1 -- one node size -- on the side the ray leaves through (`pos` bit a: toward +a)
VRC_NODE_FN uint32_t widened_box_word(unsigned axes, unsigned pos) {
    uint32_t w = 0;
    for (unsigned a = 0; a < 3; a++) w |= ((axes >> a) & 1u) << (5u * a + (((pos >> a) & 1u) ? 15u : 0u));
    return w;
}

}  // namespace vrc
