// voxel_edit.hip -- change voxels of the resident scene (vrc_set_voxels / vrc_set_voxels_device, include/vrc.h) for gfx950.
//
// A batch is sorted by (key, edit number) -- rocprim's radix sort is stable, so the edit number never enters the key -- and every
// later step works on the runs of one key, in which the LAST edit of a position wins.  Nothing depends on the order in which
// stores or atomics land: the counters are sums, the placement of every appended word is a function of the sorted keys.
//
//   voxel_edit_key_kernel     one lane per edit: the key (SVO branch: the Morton key of the edit's brick, a map-aligned 8^3 cube;
//                             array branch: the frame's index of the voxel), or the sentinel for an edit that is skipped
//   (sort by key; the unique keys in order: rocprim)
//   voxel_edit_array_kernel   array branch: the last edit of every run stores its material
//   voxel_edit_brick_kernel   SVO branch, one wave per touched brick: each lane resolves its row of 8 voxels of the OLD brick as
//                             the region read does (svo_node.hpp's node_row), the 512 materials go to LDS, the brick's run of
//                             edits is applied (an LDS max by edit number chooses the winner of a position), and the wave
//                             builds the brick's subtree from the LDS -- lane j owns the 2^3 block j = (4^3 child) << 3 | (2^3
//                             child), one ballot gives every mask and every rank -- and stores it at brick_base + 72 u, packed,
//                             with one attachment word per bottom-level descriptor.  It leaves the brick's record for its parent.
//   voxel_edit_level_kernel   one lane per touched node above the bricks, one launch per level up to the root: a child that was
//                             touched (binary search in the level below) supplies its record; an untouched child keeps its old
//                             state -- empty, a solid leaf, or its descriptor with the masks copied and a far pointer to its old
//                             child block.  The node's new child block (descriptors, then their far slots) is appended; the
//                             root's level also appends the new root word, right in front of its block.
// The edit never overwrites a word of the old tree, so the old root still decodes the old scene until the host moves the root.
// How a wave reads its old brick and how it turns the new one into a subtree live in voxel_edit_emit.hpp: the region edits'
// brick kernel (region_write.hip) ends in the same code, and the sort, the run lengths and the ancestor pass here serve it too.
#include <hip/hip_runtime.h>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_run_length_encode.hpp>

#include "svo_node.hpp"
#include "voxel_edit.h"
#include "voxel_edit_emit.hpp"
#include "vrc_launch.h"

namespace vrc {

__global__ __launch_bounds__(kEditThreads) void voxel_edit_key_kernel(const EditParams q) {
    const int64_t stride = (int64_t)gridDim.x * kEditThreads;
    for (int64_t i = (int64_t)blockIdx.x * kEditThreads + threadIdx.x; i < q.n; i += stride) {
        const int64_t x = q.positions[3 * i], y = q.positions[3 * i + 1], z = q.positions[3 * i + 2];
        const int m = q.materials[i];
        bool ok = m >= -128 && m <= 127 && x >= 0 && y >= 0 && z >= 0;
        uint64_t key = q.sentinel;
        if (q.scene.svo) {
            const int64_t dim = (int64_t)1 << q.scene.log2_dim;
            ok = ok && x < dim && y < dim && z < dim;
            if (ok) {
                key = spread3((uint64_t)x >> kReadBrickLog2) | (spread3((uint64_t)y >> kReadBrickLog2) << 1) | (spread3((uint64_t)z >> kReadBrickLog2) << 2);
                if (m != 0 && m != 5) atomicOr(&q.counters[kEditMaterials], 1ULL);
            }
        } else {
            ok = ok && x < q.scene.map_dim[0] && y < q.scene.map_dim[1] && z < q.scene.map_dim[2];
            const uint64_t idx = (uint64_t)(x + (int64_t)q.scene.map_dim[0] * (y + (int64_t)q.scene.map_dim[2] * z));
            ok = ok && idx < q.scene.map_bytes;                      // (an index past the array is skipped: the read rule)
            if (ok) key = idx;
        }
        if (!ok) atomicAdd(&q.counters[kEditSkipped], 1ULL);
        q.keys[i] = ok ? key : q.sentinel;
        q.order[i] = (uint32_t)i;
    }
}

__global__ __launch_bounds__(kEditThreads) void voxel_edit_array_kernel(const EditParams q) {
    const int64_t stride = (int64_t)gridDim.x * kEditThreads;
    for (int64_t i = (int64_t)blockIdx.x * kEditThreads + threadIdx.x; i < q.n; i += stride) {
        const uint64_t key = q.sorted_keys[i];
        if (key >= q.sentinel || (i + 1 < q.n && q.sorted_keys[i + 1] == key)) continue;     // skipped, or a later edit of this voxel follows
        const int8_t m = (int8_t)q.materials[q.sorted_order[i]];
        if (q.map[key] != m) {
            q.map[key] = m;
            atomicAdd(&q.counters[kEditChanged], 1ULL);
        }
    }
}

// shallow: the tree's depth when the brick holds the whole map (log2_dim <= 3) and the wave emits the root itself, else 0
__global__ __launch_bounds__(kEditThreads) void voxel_edit_brick_kernel(const EditParams q, const int shallow) {
    constexpr int kWaves = kEditThreads / 64;
    __shared__ uint64_t s_rows[kWaves][64];                        // the brick: row (y, z) = lane, byte x
    __shared__ uint32_t s_owner[kWaves][kEditBrickVoxels];         // per voxel: 1 + the place in the run of the last edit that writes it
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, ly = lane & 7, lz = lane >> 3;
    const int64_t u = (int64_t)blockIdx.x * kWaves + wave;
    const bool live = u < q.n_bricks;                              // (no early exit: the block's barriers are taken by every wave)
    uint64_t old_row = 0;
    int64_t first = 0, last = 0;
    if (live) {
        const uint64_t key = q.brick_keys[u];
        old_row = edit_old_row(q, key, ly, lz);
        first = lower_bound(q.sorted_keys, q.n, key);
        last = lower_bound(q.sorted_keys, q.n, key + 1);
    }
    s_rows[wave][lane] = old_row;
    for (int k = lane; k < kEditBrickVoxels; k += 64) s_owner[wave][k] = 0;
    __syncthreads();
    // the run's edits in order: the last edit of a voxel is the one with the largest place in the run
    for (int64_t i = first + lane; i < last; i += 64) {
        const int64_t e = q.sorted_order[i];
        const int v = (q.positions[3 * e] & 7) | ((q.positions[3 * e + 1] & 7) << 3) | ((q.positions[3 * e + 2] & 7) << 6);
        atomicMax(&s_owner[wave][v], (uint32_t)(i - first + 1));
    }
    __syncthreads();
    int8_t *bytes = reinterpret_cast<int8_t *>(s_rows[wave]);
    for (int64_t i = first + lane; i < last; i += 64) {
        const int64_t e = q.sorted_order[i];
        const int v = (q.positions[3 * e] & 7) | ((q.positions[3 * e + 1] & 7) << 3) | ((q.positions[3 * e + 2] & 7) << 6);
        if (s_owner[wave][v] == (uint32_t)(i - first + 1)) bytes[v] = (int8_t)q.materials[e];
    }
    __syncthreads();
    edit_emit_brick(q, shallow, u, lane, live, old_row, s_rows[wave]);
}

__global__ __launch_bounds__(kEditThreads) void voxel_edit_level_kernel(const EditParams q, const EditLevel L) {
    const int64_t i = (int64_t)blockIdx.x * kEditThreads + threadIdx.x;
    if (i >= L.count) return;
    const uint64_t key = L.keys[i];
    uint64_t cur = 0, index = 0;
    const int state = descend_to_node(q.scene, (int)(compact3(key) << L.r), (int)(compact3(key >> 1) << L.r), (int)(compact3(key >> 2) << L.r), L.r, cur, index);
    // child slot s after the edit: 0 empty, 1 a solid leaf, 2 a descriptor with `masks` whose child block starts at `target`
    auto child = [&](unsigned s, unsigned &masks, uint64_t &target) -> int {
        const uint64_t ck = (key << 3) | s;
        const int64_t at = lower_bound(L.below_keys, L.below_count, ck);
        if (at < L.below_count && L.below_keys[at] == ck) {          // touched: its record
            masks = q.rec_masks[L.rec_below + at];
            target = q.rec_child[L.rec_below + at];
            return (masks & 0xffu) ? 2 : 0;
        }
        if (state != 2) return state;                                // untouched inside an empty node / inside a solid leaf
        const unsigned old = (unsigned)cur & 0xffffu, bit = 1u << s;
        if (!(old & bit)) return 0;
        if ((old >> 8) & bit) return 1;
        const uint64_t ci = kept_child(cur, s), d = q.scene.descriptors[VRC_IDX(kDescriptors, ci)];
        masks = (unsigned)(d >> 16) & 0xffffu;
        target = ((masks & 0xffu) & ~(masks >> 8)) ? first_child(q.scene.descriptors, ci, d) : 0;   // (no descriptor below: no pointer to follow)
        return 2;
    };
    unsigned valid = 0, leaves = 0;
    for (unsigned s = 0; s < 8; s++) {
        unsigned masks = 0;
        uint64_t target = 0;
        const int kind = child(s, masks, target);
        if (kind) valid |= 1u << s;
        if (kind == 1) leaves |= 1u << s;
    }
    // the child block: a word per valid slot (a leaf's is never read and stays zero), then the far slots, rank by rank
    const uint64_t block = L.base + kEditNodeStride * (uint64_t)i + (L.root ? 1u : 0u);
    const unsigned kept = (unsigned)__builtin_popcount(valid);
    for (unsigned s = 0, rank = 0; s < 8; s++) {
        if (!(valid & (1u << s))) continue;
        unsigned masks = 0;
        uint64_t target = 0;
        if (child(s, masks, target) == 2) {
            q.descriptors[block + rank] = (uint64_t)kept | kFarBit | ((uint64_t)masks << 16);
            q.descriptors[block + kept + rank] = target;
        }
        rank++;
    }
    q.rec_masks[L.rec_here + i] = valid | ((uint32_t)leaf_bits_for(valid, leaves) << 8);
    q.rec_child[L.rec_here + i] = block;
    if (L.root) q.descriptors[L.base] = 1ULL | ((uint64_t)valid << 16) | (leaf_bits_for(valid, leaves) << 24);
}

namespace {
unsigned edit_grid_for(int64_t threads) {
    const int64_t blocks = (threads + kEditThreads - 1) / kEditThreads;
    return (unsigned)(blocks < 1 ? 1 : (blocks < (1 << 20) ? blocks : (1 << 20)));   // (larger batches: the lanes loop)
}
}  // namespace

hipError_t launch_edit_keys(const EditParams &q, hipStream_t stream) {
    (void)hipGetLastError();
    hipLaunchKernelGGL(voxel_edit_key_kernel, dim3(edit_grid_for(q.n)), dim3(kEditThreads), 0, stream, q);
    return hipGetLastError();
}

// sort n (key, edit number) pairs by the low `bits` bits of the key; temp == nullptr: *temp_bytes receives the storage needed
hipError_t edit_sort(void *temp, size_t *temp_bytes, const uint64_t *keys_in, uint64_t *keys_out, const uint32_t *order_in, uint32_t *order_out,
                     int64_t n, int bits, hipStream_t stream) {
    return rocprim::radix_sort_pairs(temp, *temp_bytes, keys_in, keys_out, order_in, order_out, (size_t)n, 0u, (unsigned)bits, stream);
}

// the unique keys of the sorted batch in order, and their number (counts: scratch of n words)
hipError_t edit_runs(void *temp, size_t *temp_bytes, const uint64_t *sorted_keys, int64_t n, uint64_t *unique, uint32_t *counts,
                     unsigned long long *n_runs, hipStream_t stream) {
    return rocprim::run_length_encode(temp, *temp_bytes, sorted_keys, (unsigned int)n, unique, counts, n_runs, stream);
}

hipError_t launch_edit_array(const EditParams &q, hipStream_t stream) {
    (void)hipGetLastError();
    hipLaunchKernelGGL(voxel_edit_array_kernel, dim3(edit_grid_for(q.n)), dim3(kEditThreads), 0, stream, q);
    return hipGetLastError();
}

hipError_t launch_edit_bricks(const EditParams &q, hipStream_t stream) {
    (void)hipGetLastError();
    const int64_t blocks = (q.n_bricks + kEditThreads / 64 - 1) / (kEditThreads / 64);
    if (blocks < 1 || blocks > 0x7fffffffLL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(voxel_edit_brick_kernel, dim3((unsigned)blocks), dim3(kEditThreads), 0, stream, q, q.scene.log2_dim <= kReadBrickLog2 ? q.scene.log2_dim : 0);
    return hipGetLastError();
}

hipError_t launch_edit_level(const EditParams &q, const EditLevel &level, hipStream_t stream) {
    (void)hipGetLastError();
    const int64_t blocks = (level.count + kEditThreads - 1) / kEditThreads;
    if (blocks < 1 || blocks > 0x7fffffffLL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(voxel_edit_level_kernel, dim3((unsigned)blocks), dim3(kEditThreads), 0, stream, q, level);
    return hipGetLastError();
}

}  // namespace vrc

VRC_AUDIT_TU(edit)
