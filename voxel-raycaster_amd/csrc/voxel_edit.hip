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
#include <hip/hip_runtime.h>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_run_length_encode.hpp>

#include "svo_node.hpp"
#include "voxel_edit.h"
#include "vrc_launch.h"

namespace vrc {

namespace {

// bit k of v to bit 3 k (21 bits), and back
__host__ __device__ inline uint64_t spread3(uint64_t x) {
    x &= 0x1fffffULL;
    x = (x | x << 32) & 0x1f00000000ffffULL;
    x = (x | x << 16) & 0x1f0000ff0000ffULL;
    x = (x | x << 8) & 0x100f00f00f00f00fULL;
    x = (x | x << 4) & 0x10c30c30c30c30c3ULL;
    x = (x | x << 2) & 0x1249249249249249ULL;
    return x;
}
__host__ __device__ inline uint32_t compact3(uint64_t x) {
    x &= 0x1249249249249249ULL;
    x = (x ^ (x >> 2)) & 0x10c30c30c30c30c3ULL;
    x = (x ^ (x >> 4)) & 0x100f00f00f00f00fULL;
    x = (x ^ (x >> 8)) & 0x1f0000ff0000ffULL;
    x = (x ^ (x >> 16)) & 0x1f00000000ffffULL;
    x = (x ^ (x >> 32)) & 0x1fffffULL;
    return (uint32_t)x;
}

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

}  // namespace

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
        const int ox = (int)(compact3(key) << kReadBrickLog2), oy = (int)(compact3(key >> 1) << kReadBrickLog2), oz = (int)(compact3(key >> 2) << kReadBrickLog2);
        const int n = q.scene.log2_dim;
        if (n >= kReadBrickLog2) {
            uint64_t cur = 0, index = 0;
            const int state = descend_to_node(q.scene, ox, oy, oz, kReadBrickLog2, cur, index);
            if (state == 1) old_row = 0x0505050505050505ULL;
            if (state == 2) old_row = node_row<3>(q.scene, cur, index, ly, lz);
        } else if (ly < (1 << n) && lz < (1 << n)) {
            const uint64_t cur = node_entry(q.scene.descriptors, q.scene.root_index, q.scene.descriptors[VRC_IDX(kDescriptors, q.scene.root_index)]);
            old_row = n == 2 ? node_row<2>(q.scene, cur, q.scene.root_index, ly, lz) : node_row<1>(q.scene, cur, q.scene.root_index, ly, lz);
        }
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
    // voxels whose material differs after the batch
    {
        const uint64_t diff = old_row ^ s_rows[wave][lane];
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
