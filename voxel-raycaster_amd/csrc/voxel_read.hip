// voxel_read.hip -- read voxels back from the resident scene (vrc_get_voxels / vrc_read_regions, include/vrc.h) for gfx950.
//
// The material of a voxel is the box queries' (box_walk.hpp): the array branch reads the byte at the frame's index; the SVO
// branch finds the voxel solid in a valid leaf slot at any level or in any valid slot at the bottom level, with the attachment
// byte for bottom-level descriptors when attachments are assigned, else 5.  Outside the map is 0.  One launch per call: no plan
// pass, no scan, no scratch, no LDS.
//
//   voxel_points_kernel    one lane per point: svo_node.hpp's descent (from the coarse cell when the table is there) taken
//                          down to the voxel
//   voxel_regions_kernel   one wave per (region, brick): a brick is a map-aligned 8^3 cube, one level-3 node.  A region touches
//                          at most (size + 6) / 8 + 1 bricks per axis whatever its alignment, so the waves are numbered over
//                          n x bx x by x bz and a wave whose brick misses its region leaves.  The wave descends ONCE to the
//                          brick's node -- everything up to there is a function of the wave's number, formed through
//                          readfirstlane, so the descent's loads are scalar loads -- and lane (y, z) of the brick then resolves its
//                          own row of 8 voxels along x from the two levels of descriptors under the node.  A lane stores the part
//                          of its row that lies in the region: one 8-byte store when the row is whole and lands 8-byte aligned,
//                          byte stores otherwise, never a read-modify-write (the neighbouring bytes are other waves').
#include <hip/hip_runtime.h>

#include "svo_node.hpp"
#include "voxel_read.h"
#include "vrc_launch.h"

namespace vrc {

namespace {

// array branch: voxels (x .. x + 7, y, z) by the frame's index (y stride map_dim[2]); past the array and outside map_dim reads as 0
__device__ __forceinline__ uint64_t array_row(const ReadParams &q, int64_t x, int64_t y, int64_t z) {
    if (y < 0 || y >= q.scene.map_dim[1] || z < 0 || z >= q.scene.map_dim[2]) return 0;
    const int64_t base = x + (int64_t)q.scene.map_dim[0] * (y + (int64_t)q.scene.map_dim[2] * z);
    if (x >= 0 && x + 8 <= q.scene.map_dim[0] && (uint64_t)base + 8u <= q.scene.map_bytes && (((uintptr_t)q.scene.map + (uint64_t)base) & 7u) == 0)
        return *reinterpret_cast<const uint64_t *>(q.scene.map + base);
    uint64_t row = 0;
    for (int k = 0; k < 8; k++) {
        const int64_t xx = x + k;
        const uint64_t idx = (uint64_t)(base + k);
        if (xx >= 0 && xx < q.scene.map_dim[0] && idx < q.scene.map_bytes) row |= (uint64_t)(uint8_t)q.scene.map[VRC_IDX(kMap, idx)] << (8 * k);
    }
    return row;
}

__device__ __forceinline__ int64_t uniform64(int64_t v) {
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)(uint64_t)v), hi = __builtin_amdgcn_readfirstlane((uint32_t)((uint64_t)v >> 32));
    return (int64_t)(((uint64_t)hi << 32) | lo);
}

}  // namespace

__global__ __launch_bounds__(kReadThreads) void voxel_points_kernel(const ReadParams q) {
    const int64_t stride = (int64_t)gridDim.x * kReadThreads;
    for (int64_t i = (int64_t)blockIdx.x * kReadThreads + threadIdx.x; i < q.n; i += stride) {
        const int x = q.positions[3 * i], y = q.positions[3 * i + 1], z = q.positions[3 * i + 2];
        int mat = 0;
        if (q.scene.svo) {
            const int dim = 1 << q.scene.log2_dim;
            if (x >= 0 && y >= 0 && z >= 0 && x < dim && y < dim && z < dim) mat = voxel_material(q.scene, x, y, z);
        } else if (x >= 0 && y >= 0 && z >= 0 && x < q.scene.map_dim[0] && y < q.scene.map_dim[1] && z < q.scene.map_dim[2]) {
            const uint64_t idx = (uint64_t)((int64_t)x + (int64_t)q.scene.map_dim[0] * ((int64_t)y + (int64_t)q.scene.map_dim[2] * z));
            mat = idx < q.scene.map_bytes ? (int)q.scene.map[VRC_IDX(kMap, idx)] : 0;
        }
        q.values[i] = mat;
    }
}

__global__ __launch_bounds__(kReadThreads) void voxel_regions_kernel(const ReadParams q) {
    constexpr int kWaves = kReadThreads / 64, kBrick = 1 << kReadBrickLog2;
    const int lane = threadIdx.x & 63, ly = lane & 7, lz = lane >> 3;
    const int64_t per_region = q.bricks[0] * q.bricks[1] * q.bricks[2], waves = q.n * per_region;
    const int64_t sx = q.size[0], sy = q.size[1], sz = q.size[2];
    // One item per wave and no loop over items: every load of the kernel then comes before its first store, which is what lets
    // the compiler take the wave-uniform ones (the corner, the descent) as scalar loads.
    const int64_t block = ((int64_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    const int64_t w = uniform64(block * kWaves + threadIdx.x / 64);
    if (w < waves) {
        const int64_t region = w / per_region;
        int64_t k = w - region * per_region;
        const int64_t jx = k % q.bricks[0];
        k /= q.bricks[0];
        const int64_t jy = k % q.bricks[1], jz = k / q.bricks[1];
        const int64_t lo_x = q.positions[3 * region], lo_y = q.positions[3 * region + 1], lo_z = q.positions[3 * region + 2];
        // the brick's origin (64 bits: lo is any int32) and where it sits in the region
        const int64_t ox = ((lo_x >> kReadBrickLog2) + jx) * kBrick, oy = ((lo_y >> kReadBrickLog2) + jy) * kBrick, oz = ((lo_z >> kReadBrickLog2) + jz) * kBrick;
        if (ox >= lo_x + sx || oy >= lo_y + sy || oz >= lo_z + sz) return;              // the brick misses its region
        uint64_t row = 0;
        if (q.scene.svo) {
            const int n = q.scene.log2_dim;
            const int64_t dim = (int64_t)1 << n;
            // (a brick wholly outside the map writes its zeros without touching the tree)
            if (ox >= 0 && oy >= 0 && oz >= 0 && ox < dim && oy < dim && oz < dim) {
                if (n >= kReadBrickLog2) {
                    uint64_t cur = 0, index = 0;
                    const int state = descend_to_node(q.scene, (int)ox, (int)oy, (int)oz, kReadBrickLog2, cur, index);
                    if (state == 1) row = 0x0505050505050505ULL;
                    if (state == 2) row = node_row<3>(q.scene, cur, index, ly, lz);
                } else if (ly < dim && lz < dim) {
                    // a tree shallower than a brick: the brick at the origin holds the whole map, the rest of it is outside
                    const uint64_t cur = node_entry(q.scene.descriptors, q.scene.root_index, q.scene.descriptors[VRC_IDX(kDescriptors, q.scene.root_index)]);
                    row = n == 2 ? node_row<2>(q.scene, cur, q.scene.root_index, ly, lz) : node_row<1>(q.scene, cur, q.scene.root_index, ly, lz);
                }
            }
        } else if (ox + kBrick > 0 && oy + kBrick > 0 && oz + kBrick > 0 && ox < q.scene.map_dim[0] && oy < q.scene.map_dim[1] && oz < q.scene.map_dim[2]) {
            row = array_row(q, ox, oy + ly, oz + lz);
        }
        // the part of the row inside the region
        const int64_t ry = oy + ly - lo_y, rz = oz + lz - lo_z, rx = ox - lo_x;
        if (ry < 0 || ry >= sy || rz < 0 || rz >= sz) return;
        const int k0 = rx < 0 ? (int)-rx : 0, k1 = sx - rx < kBrick ? (int)(sx - rx) : kBrick;
        int8_t *dst = q.bytes + ((size_t)region * (size_t)sx * (size_t)sy * (size_t)sz + (size_t)(sx * (ry + sy * rz)) + (size_t)(rx + k0));
        if (k0 == 0 && k1 == kBrick && ((uintptr_t)dst & 7u) == 0) {
            *reinterpret_cast<uint64_t *>(dst) = row;
        } else {
#pragma clang loop vectorize(disable)
            for (int b = k0; b < k1; b++) dst[b - k0] = (int8_t)(row >> (8 * b));
        }
    }
}

namespace {
unsigned read_grid_for(int64_t threads) {
    const int64_t blocks = (threads + kReadThreads - 1) / kReadThreads;
    return (unsigned)(blocks < 1 ? 1 : (blocks < (1 << 20) ? blocks : (1 << 20)));   // (larger batches: the lanes loop)
}
}  // namespace

hipError_t launch_voxel_points(const ReadParams &q, hipStream_t stream) {
    (void)hipGetLastError();
    hipLaunchKernelGGL(voxel_points_kernel, dim3(read_grid_for(q.n)), dim3(kReadThreads), 0, stream, q);
    return hipGetLastError();
}

hipError_t launch_voxel_regions(const ReadParams &q, hipStream_t stream) {
    (void)hipGetLastError();
    // one wave per (region, brick); past 2^22 blocks the grid's other two dimensions carry the rest
    const int64_t waves = q.n * q.bricks[0] * q.bricks[1] * q.bricks[2], blocks = (waves + kReadThreads / 64 - 1) / (kReadThreads / 64);
    const int64_t gx = blocks < (1 << 22) ? blocks : (1 << 22), rows = (blocks + gx - 1) / gx;
    const int64_t gy = rows < 65535 ? rows : 65535, gz = (rows + gy - 1) / gy;
    if (gz > 65535) return hipErrorInvalidValue;
    hipLaunchKernelGGL(voxel_regions_kernel, dim3((unsigned)gx, (unsigned)gy, (unsigned)gz), dim3(kReadThreads), 0, stream, q);
    return hipGetLastError();
}

}  // namespace vrc

VRC_AUDIT_TU(read)
