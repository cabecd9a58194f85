// octree_compact.hip -- copy what the root reaches into a new, dense, canonically ordered array (vrc_compact_octree,
// include/vrc.h) for gfx950.
//
// The new array is pre-order: the root at 0, then for every descriptor that holds a pointer its child block (the children, the
// far slots of its far children), then the children's own blocks in child order.  The placement of every word is a function of
// the subtree sizes alone, so three sweeps over per-level lists do it, one launch per level, and no atomic decides a place:
//
//   octree_compact_count_kernel     gather, top-down, a lane per list entry: which children hold a pointer (pmask) and how many
//   (exclusive scan of the counts: rocprim)
//   octree_compact_scatter_kernel   ... the next level's list: child `rank` of entry i is entry scan[i] + rank
//   octree_compact_size_kernel      sizes, bottom-up: S = m + f + sum of the children's S, a child far when 16 + the S of the
//                                   children before it exceeds the reach (farmask)
//   octree_compact_root_kernel      emit: word 0
//   octree_compact_emit_kernel      emit, top-down: an entry receives its block's start B from its parent, stores the block (bits
//                                   16-63 of the old words, the new pointers), the far slots and the lookup words of bottom-level
//                                   children, hands T_k to its children and raises the used flags of the attachment slots
//   (exclusive scan of the used flags: rocprim)
//   octree_compact_lookup_kernel    a lane per new word: old slot -> new slot
//   octree_compact_attach_kernel    a lane per old slot: a used slot's word goes to its new place
// The lists end one level above the bottom: bottom-level descriptors are copied with their parent's block.  An index outside
// the old tree or the new array is counted (kCompactBad) and not accessed; the host fails the call then.
#include <hip/hip_runtime.h>

#include <rocprim/device/device_scan.hpp>

#include "octree_compact.h"
#include "svo_node.hpp"
#include "vrc_launch.h"

namespace vrc {

namespace {

__device__ inline void bad_index(const CompactParams &q) { atomicAdd(&q.counters[kCompactBad], 1ULL); }

// word `index` of the old tree (0 and counted when there is no such word)
__device__ inline uint64_t old_word(const CompactParams &q, uint64_t index) {
    if (index >= q.n_old) { bad_index(q); return 0; }
    return q.scene.descriptors[VRC_IDX(kDescriptors, index)];
}

// first kept child of the old descriptor d at `index` (n_old and counted when its far slot lies outside the array)
__device__ inline uint64_t old_block(const CompactParams &q, uint64_t index, uint64_t d) {
    if ((d & kFarBit) && index + (d & kNearMask) >= q.n_old) { bad_index(q); return q.n_old; }
    return first_child(q.scene.descriptors, index, d);
}

// (a dry run has no new array: out == nullptr, and nothing is stored)
__device__ inline void store_word(const CompactParams &q, uint64_t index, uint64_t v) {
    if (!q.out) return;
    if (index < q.n_out) q.out[index] = v; else bad_index(q);
}

// the lookup word of the bottom-level descriptor at old index `index`, whose slot is raised as used
__device__ inline uint32_t take_slot(const CompactParams &q, uint64_t index) {
    if (index >= q.n_old) return 0;                                // (counted by the read of the descriptor itself)
    const uint32_t slot = q.scene.attach_lookup[VRC_IDX(kAttachLookup, index)];
    if (slot >= q.n_attach_old) { bad_index(q); return 0; }
    q.used[slot] = 1;
    return slot;
}

}  // namespace

__global__ __launch_bounds__(kCompactThreads) void octree_compact_count_kernel(const CompactParams q, const CompactLevel L) {
    const int64_t i = (int64_t)blockIdx.x * kCompactThreads + threadIdx.x;
    if (i > L.count) return;
    if (i == L.count) { L.cnt[i] = 0; return; }
    const uint64_t at = L.list[i], d = old_word(q, at);
    const unsigned valid = (unsigned)(d >> 16) & 0xffu, leaf = (unsigned)(d >> 24) & 0xffu;
    unsigned pmask = 0;
    if (!L.children_bottom) {
        const uint64_t block = old_block(q, at, d);
#pragma unroll
        for (unsigned k = 0; k < 8; k++) {
            const unsigned bit = 1u << k;
            if ((valid & ~leaf) & bit)
                if ((old_word(q, block + child_rank(valid, k)) >> 16) & 0xffULL) pmask |= bit;
        }
    }
    L.pmask[i] = (uint8_t)pmask;
    L.cnt[i] = (uint64_t)__builtin_popcount(pmask);
}

__global__ __launch_bounds__(kCompactThreads) void octree_compact_scatter_kernel(const CompactParams q, const CompactLevel L) {
    const int64_t i = (int64_t)blockIdx.x * kCompactThreads + threadIdx.x;
    if (i >= L.count) return;
    const unsigned pmask = L.pmask[i];
    if (!pmask) return;
    const uint64_t at = L.list[i], d = old_word(q, at);
    const unsigned valid = (unsigned)(d >> 16) & 0xffu;
    const uint64_t block = old_block(q, at, d);
    uint64_t to = L.scan[i];
#pragma unroll
    for (unsigned k = 0; k < 8; k++)
        if (pmask & (1u << k)) L.next_list[to++] = block + child_rank(valid, k);
}

__global__ __launch_bounds__(kCompactThreads) void octree_compact_size_kernel(const CompactParams q, const CompactLevel L) {
    const int64_t i = (int64_t)blockIdx.x * kCompactThreads + threadIdx.x;
    if (i >= L.count) return;
    const uint64_t d = old_word(q, L.list[i]);
    const unsigned valid = (unsigned)(d >> 16) & 0xffu, pmask = L.pmask[i];
    uint64_t below = 0, from = pmask ? L.scan[i] : 0;
    unsigned farmask = 0;
#pragma unroll
    for (unsigned k = 0; k < 8; k++) {
        if (!(pmask & (1u << k))) continue;
        if (16 + below > q.reach) farmask |= 1u << k;
        below += L.size_below[from++];
    }
    const unsigned far = (unsigned)__builtin_popcount(farmask);
    L.farmask[i] = (uint8_t)farmask;
    L.size[i] = (uint64_t)__builtin_popcount(valid) + far + below;
    if (far) atomicAdd(&q.counters[kCompactFar], (unsigned long long)far);
}

__global__ void octree_compact_root_kernel(const CompactParams q) {
    if (blockIdx.x || threadIdx.x) return;
    const uint64_t d = old_word(q, q.scene.root_index);
    const bool bottom = q.scene.log2_dim <= 1;
    store_word(q, 0, (d & ~0xffffULL) | ((!bottom && ((d >> 16) & 0xffULL)) ? 1ULL : 0ULL));
    if (q.used && bottom) {
        const uint32_t slot = take_slot(q, q.scene.root_index);
        if (q.out_lookup) q.out_lookup[0] = slot;
    }
}

__global__ __launch_bounds__(kCompactThreads) void octree_compact_emit_kernel(const CompactParams q, const CompactLevel L) {
    const int64_t i = (int64_t)blockIdx.x * kCompactThreads + threadIdx.x;
    if (i >= L.count) return;
    const uint64_t at = L.list[i], d = old_word(q, at);
    const unsigned valid = (unsigned)(d >> 16) & 0xffu, leaf = (unsigned)(d >> 24) & 0xffu, pmask = L.pmask[i], farmask = L.farmask[i];
    const uint64_t block = old_block(q, at, d);
    const uint64_t base = L.base[i], kept = (uint64_t)__builtin_popcount(valid);
    uint64_t slot = base + kept;                                   // the next far slot
    uint64_t target = slot + (uint64_t)__builtin_popcount(farmask);    // T_k: where the next pointer-holding child's block starts
    uint64_t from = pmask ? L.scan[i] : 0;
#pragma unroll
    for (unsigned k = 0; k < 8; k++) {
        const unsigned bit = 1u << k;
        if (!(valid & bit)) continue;
        const unsigned rank = child_rank(valid, k);
        const uint64_t child = block + rank, to = base + rank;
        uint64_t w = old_word(q, child) & ~0xffffULL;
        if (pmask & bit) {
            if (farmask & bit) {
                store_word(q, slot, target);
                w |= kFarBit | (slot - to);
                slot++;
            } else {
                w |= target - to;
            }
            L.base_below[from] = target;
            target += L.size_below[from];
            from++;
        }
        store_word(q, to, w);
        if (q.used && L.children_bottom && !(leaf & bit)) {
            const uint32_t named = take_slot(q, child);
            if (q.out_lookup && to < q.n_out) q.out_lookup[to] = named;
        }
    }
}

__global__ __launch_bounds__(kCompactThreads) void octree_compact_lookup_kernel(uint32_t *lookup, uint64_t n, const uint64_t *remap) {
    const uint64_t i = (uint64_t)blockIdx.x * kCompactThreads + threadIdx.x;
    if (i < n) lookup[i] = (uint32_t)remap[lookup[i]];            // (a word that is no bottom-level descriptor holds 0, and remap[0] = 0)
}

__global__ __launch_bounds__(kCompactThreads) void octree_compact_attach_kernel(const CompactParams q, const uint64_t *remap, uint64_t *attach, uint64_t n_new) {
    const uint64_t i = (uint64_t)blockIdx.x * kCompactThreads + threadIdx.x;
    if (i >= q.n_attach_old || !q.used[i]) return;
    const uint64_t to = remap[i];
    if (to < n_new) attach[to] = q.scene.attachments[VRC_IDX(kAttachments, i)]; else bad_index(q);
}

namespace {
// a lane per item; false when the grid would not fit
bool compact_grid(uint64_t items, unsigned *blocks) {
    const uint64_t b = (items + kCompactThreads - 1) / kCompactThreads;
    *blocks = (unsigned)(b < 1 ? 1 : b);
    return b <= 0x7fffffffULL;
}
}  // namespace

// pass: 0 count, 1 scatter, 2 sizes, 3 emit
hipError_t launch_compact_level(const CompactParams &q, const CompactLevel &level, int pass, hipStream_t stream) {
    (void)hipGetLastError();
    unsigned blocks = 1;
    if (level.count < 1 || !compact_grid((uint64_t)level.count + (pass == 0 ? 1 : 0), &blocks)) return hipErrorInvalidValue;
    if (pass == 0) hipLaunchKernelGGL(octree_compact_count_kernel, dim3(blocks), dim3(kCompactThreads), 0, stream, q, level);
    else if (pass == 1) hipLaunchKernelGGL(octree_compact_scatter_kernel, dim3(blocks), dim3(kCompactThreads), 0, stream, q, level);
    else if (pass == 2) hipLaunchKernelGGL(octree_compact_size_kernel, dim3(blocks), dim3(kCompactThreads), 0, stream, q, level);
    else hipLaunchKernelGGL(octree_compact_emit_kernel, dim3(blocks), dim3(kCompactThreads), 0, stream, q, level);
    return hipGetLastError();
}

hipError_t launch_compact_root(const CompactParams &q, hipStream_t stream) {
    (void)hipGetLastError();
    hipLaunchKernelGGL(octree_compact_root_kernel, dim3(1), dim3(64), 0, stream, q);
    return hipGetLastError();
}

// the materials: the new lookup's n_new words from old slots to new ones, the used slots' words to `attach` (n_attach_new words)
hipError_t launch_compact_materials(const CompactParams &q, const uint64_t *remap, uint64_t n_new, uint64_t *attach, uint64_t n_attach_new, hipStream_t stream) {
    (void)hipGetLastError();
    unsigned blocks = 1;
    if (!compact_grid(n_new, &blocks)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(octree_compact_lookup_kernel, dim3(blocks), dim3(kCompactThreads), 0, stream, q.out_lookup, n_new, remap);
    if (!compact_grid(q.n_attach_old, &blocks)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(octree_compact_attach_kernel, dim3(blocks), dim3(kCompactThreads), 0, stream, q, remap, attach, n_attach_new);
    return hipGetLastError();
}

// exclusive scan of n words (rocprim); temp == nullptr: *temp_bytes receives the storage it needs
hipError_t compact_scan(void *temp, size_t *temp_bytes, const uint64_t *in, uint64_t *out, uint64_t n, hipStream_t stream) {
    return rocprim::exclusive_scan(temp, *temp_bytes, in, out, (uint64_t)0, (size_t)n, rocprim::plus<uint64_t>(), stream);
}

}  // namespace vrc

VRC_AUDIT_TU(compact)
