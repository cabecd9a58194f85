// face_extract.hip -- the exposed voxel faces of the resident scene (vrc_extract_faces, include/vrc.h) for gfx950.
//
// Face (v, d) exists when voxel v is solid, lies in its region and in the scene, and the neighbour v + e_d (d = 0 .. 5: -x, +x,
// -y, +y, -z, +z) is not solid.  The neighbour is read from the SCENE, not from the region, so regions that tile the map give
// disjoint face sets whose union is the map's; a neighbour outside the scene is empty.  The material of a voxel is the voxel
// reads' (voxel_read.hip).  No atomic decides a place or a value, nothing is sorted: the list order IS the wave numbering and
// then the lane order.
//
//   face_count_kernel     one wave per (region, brick), numbered as in voxel_regions_kernel: one scalar descent to the brick's
//                         node, lane (y, z) holds its row of 8 materials along x and forms six 8-bit exposure masks -- +-x from
//                         the row shifted by one voxel plus one bit of the +-x neighbour brick's row, +-y and +-z from the rows
//                         of lanes +-1 and +-8 by cross-lane moves; the lanes on a brick face take their row from the neighbour
//                         brick's node, at most six further wave-uniform descents, each skipped when no lane owns a solid voxel
//                         on that brick face.  A brick that misses its region or the scene, or owns no solid voxel, leaves
//                         before any neighbour is looked at.  The wave's total goes to item_count.
//   (inclusive scan of the item counts over all the items: rocprim, box_scan)
//   face_region_kernel    one lane per region: counts[i] from the scan, with plain stores
//   face_emit_kernel      capacity > 0 only: the waves whose first face lies below `capacity` form their masks again; a lane's
//                         place is the wave's start plus the exclusive scan of the lane counts, its entries go out x-ascending,
//                         then d-ascending, and every store is bounded by `capacity`.
// No LDS, no scratch.
#include <hip/hip_runtime.h>

#include "face_extract.h"
#include "svo_node.hpp"
#include "vrc_launch.h"

namespace vrc {

namespace {

constexpr int kBrick = 1 << kFaceBrickLog2;

// array branch: voxels (x .. x + 7, y, z) by the frame's index (y stride map_dim[2]); past the array and outside map_dim reads as 0
__device__ __forceinline__ uint64_t map_row(const SceneView &s, int64_t x, int64_t y, int64_t z) {
    if (y < 0 || y >= s.map_dim[1] || z < 0 || z >= s.map_dim[2]) return 0;
    const int64_t base = x + (int64_t)s.map_dim[0] * (y + (int64_t)s.map_dim[2] * z);
    if (x >= 0 && x + 8 <= s.map_dim[0] && (uint64_t)base + 8u <= s.map_bytes && (((uintptr_t)s.map + (uint64_t)base) & 7u) == 0)
        return *reinterpret_cast<const uint64_t *>(s.map + VRC_IDX_N(kMap, (uint64_t)base, 8));
    uint64_t row = 0;
    for (int k = 0; k < 8; k++) {
        const int64_t xx = x + k;
        const uint64_t idx = (uint64_t)(base + k);
        if (xx >= 0 && xx < s.map_dim[0] && idx < s.map_bytes) row |= (uint64_t)(uint8_t)s.map[VRC_IDX(kMap, idx)] << (8 * k);
    }
    return row;
}

__device__ __forceinline__ int64_t uniform64(int64_t v) {
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)(uint64_t)v), hi = __builtin_amdgcn_readfirstlane((uint32_t)((uint64_t)v >> 32));
    return (int64_t)(((uint64_t)hi << 32) | lo);
}

// The brick at the map-aligned origin (ox, oy, oz), wave-uniform: 0 it is empty or outside the scene, 1 solid throughout
// (material 5), 2 a level-3 node (cur, index), 3 the root of a tree shallower than a brick (the brick at the origin holds the
// whole map), 4 a brick of the dense map.
struct Brick { int state; uint64_t cur, index; };
__device__ __forceinline__ Brick find_brick(const SceneView &s, int64_t ox, int64_t oy, int64_t oz) {
    Brick b = {0, 0, 0};
    if (ox < 0 || oy < 0 || oz < 0 || ox >= s.map_dim[0] || oy >= s.map_dim[1] || oz >= s.map_dim[2]) return b;
    if (!s.svo) {
        b.state = 4;
    } else if (s.log2_dim >= kFaceBrickLog2) {
        b.state = descend_to_node(s, (int)ox, (int)oy, (int)oz, kFaceBrickLog2, b.cur, b.index);
    } else {
        b.index = s.root_index;
        b.cur = node_entry(s.descriptors, s.root_index, s.descriptors[VRC_IDX(kDescriptors, s.root_index)]);
        b.state = 3;
    }
    return b;
}

// row (y, z) of the brick, one material per byte, lowest x first (y, z in 0 .. 7; state != 0)
__device__ __forceinline__ uint64_t brick_row(const SceneView &s, const Brick &b, int64_t ox, int64_t oy, int64_t oz, int y, int z) {
    if (b.state == 4) return map_row(s, ox, oy + y, oz + z);
    if (b.state == 1) return 0x0505050505050505ULL;
    if (b.state == 2) return node_row<3>(s, b.cur, b.index, y, z);
    const int dim = 1 << s.log2_dim;
    if (y >= dim || z >= dim) return 0;
    return s.log2_dim == 2 ? node_row<2>(s, b.cur, b.index, y, z) : node_row<1>(s, b.cur, b.index, y, z);
}

// bit k: voxel k of the row is solid (non-zero; stopping: material 5 or 6, what the renderer draws)
__device__ __forceinline__ unsigned solid_bits(uint64_t row, bool stopping) {
    unsigned m = 0;
#pragma unroll
    for (int k = 0; k < 8; k++) {
        const unsigned v = (unsigned)(row >> (8 * k)) & 0xffu;
        m |= (unsigned)(stopping ? (v == 5u || v == 6u) : v != 0u) << k;
    }
    return m;
}

// The faces lane (y, z) of item w owns: bit 8 d + k = face d of voxel (ox + k, y, z), whose materials are `row`.  0 in every
// lane when the brick owns none.  Every lane of the wave calls this (cross-lane moves); w is wave-uniform.
__device__ __forceinline__ uint64_t brick_faces(const FaceParams &q, int64_t w, int lane, int64_t &ox, int64_t &y, int64_t &z, uint64_t &row) {
    const int ly = lane & 7, lz = lane >> 3;
    const bool stopping = (q.flags & kFacesStoppingOnly) != 0;
    const int64_t per_region = q.bricks[0] * q.bricks[1] * q.bricks[2];
    const int64_t sx = q.size[0], sy = q.size[1], sz = q.size[2];
    const int64_t region = w / per_region;
    int64_t k = w - region * per_region;
    const int64_t jx = k % q.bricks[0];
    k /= q.bricks[0];
    const int64_t jy = k % q.bricks[1], jz = k / q.bricks[1];
    const int64_t lo_x = q.lo[3 * region], lo_y = q.lo[3 * region + 1], lo_z = q.lo[3 * region + 2];
    // the brick's origin (64 bits: lo is any int32)
    ox = ((lo_x >> kFaceBrickLog2) + jx) * kBrick;
    const int64_t oy = ((lo_y >> kFaceBrickLog2) + jy) * kBrick, oz = ((lo_z >> kFaceBrickLog2) + jz) * kBrick;
    y = oy + ly; z = oz + lz; row = 0;
    if (ox >= lo_x + sx || oy >= lo_y + sy || oz >= lo_z + sz) return 0;                // the brick misses its region
    const Brick own = find_brick(q.scene, ox, oy, oz);
    if (own.state == 0) return 0;                                                       // outside the scene, or empty
    row = brick_row(q.scene, own, ox, oy, oz, ly, lz);
    const unsigned s = solid_bits(row, stopping);
    // the owners: the solid voxels of the row inside the region (outside the scene nothing is solid)
    const int k0 = lo_x > ox ? (int)(lo_x - ox) : 0, k1 = lo_x + sx - ox < kBrick ? (int)(lo_x + sx - ox) : kBrick;
    const bool in_yz = y >= lo_y && y < lo_y + sy && z >= lo_z && z < lo_z + sz;
    const unsigned owner = in_yz ? s & ((1u << k1) - (1u << k0)) : 0u;
    if (__ballot(owner != 0u) == 0ULL) return 0;                                        // the brick owns no solid voxel
    const bool edges = (q.flags & kFacesNoMapEdge) == 0;
    uint64_t faces = 0;
#pragma unroll 1
    for (int d = 0; d < 6; d++) {
        const int axis = d >> 1, up = d & 1;
        // the lanes on this face of the brick, the row of the neighbour brick they look at, and that brick
        const bool at_face = axis == 0 ? ((owner >> (up ? 7 : 0)) & 1u) != 0u : (owner != 0u && (axis == 1 ? ly : lz) == (up ? 7 : 0));
        const int fy = axis == 1 ? (up ? 0 : 7) : ly, fz = axis == 2 ? (up ? 0 : 7) : lz;
        const int64_t step = up ? kBrick : -kBrick;
        const int64_t nx = ox + (axis == 0 ? step : 0), ny = oy + (axis == 1 ? step : 0), nz = oz + (axis == 2 ? step : 0);
        unsigned beyond = 0;                                                            // the solid bits of that row
        if (__ballot(at_face) != 0ULL) {
            const Brick nb = find_brick(q.scene, nx, ny, nz);
            if (nb.state != 0 && at_face) beyond = solid_bits(brick_row(q.scene, nb, nx, ny, nz, fy, fz), stopping);
        }
        // the neighbours' solid bits, and the voxels of the row whose neighbour lies outside the scene
        unsigned next, outside;
        if (axis == 0) {
            next = up ? (s >> 1) | ((beyond & 1u) << 7) : ((s << 1) & 0xffu) | (beyond >> 7);
            const int64_t edge = up ? (int64_t)q.scene.map_dim[0] - 1 - ox : -ox;       // the voxel of the row at the map's side
            outside = edge >= 0 && edge < kBrick ? 1u << (int)edge : 0u;
        } else {
            const unsigned inner = (unsigned)__shfl((int)s, (lane + (axis == 1 ? 1 : 8) * (up ? 1 : -1)) & 63);
            next = (axis == 1 ? ly : lz) == (up ? 7 : 0) ? beyond : inner;
            const int64_t at = axis == 1 ? y : z, last = (int64_t)q.scene.map_dim[axis] - 1;
            outside = (up ? at == last : at == 0) ? 0xffu : 0u;
        }
        unsigned m = owner & ~next;
        if (!edges) m &= ~outside;
        faces |= (uint64_t)m << (8 * d);
    }
    return faces;
}

}  // namespace

__global__ __launch_bounds__(kFaceThreads) void face_count_kernel(const FaceParams q) {
    constexpr int kWaves = kFaceThreads / 64;
    const int lane = threadIdx.x & 63;
    const int64_t items = q.n * q.bricks[0] * q.bricks[1] * q.bricks[2];
    const int64_t block = ((int64_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    const int64_t w = uniform64(block * kWaves + threadIdx.x / 64);
    if (w >= items) return;
    int64_t ox, y, z;
    uint64_t row;
    const uint64_t faces = brick_faces(q, w, lane, ox, y, z, row);
    int total = 0;
    if (__ballot(faces != 0ULL) != 0ULL) {
        total = __popcll(faces);
        for (int o = 32; o > 0; o >>= 1) total += __shfl_xor(total, o);
    }
    if (lane == 0) q.item_count[w] = total;
}

__global__ __launch_bounds__(kFaceThreads) void face_region_kernel(const FaceParams q) {
    const int64_t per_region = q.bricks[0] * q.bricks[1] * q.bricks[2];
    const int64_t i = (int64_t)blockIdx.x * kFaceThreads + threadIdx.x;
    if (i >= q.n) return;
    const int64_t end = q.item_end[(i + 1) * per_region - 1], start = i > 0 ? q.item_end[i * per_region - 1] : 0;
    q.counts[i] = end - start;
}

__global__ __launch_bounds__(kFaceThreads) void face_emit_kernel(const FaceParams q) {
    constexpr int kWaves = kFaceThreads / 64;
    const int lane = threadIdx.x & 63;
    const int64_t items = q.n * q.bricks[0] * q.bricks[1] * q.bricks[2];
    const int64_t block = ((int64_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    const int64_t w = uniform64(block * kWaves + threadIdx.x / 64);
    if (w >= items) return;
    const int64_t end = uniform64(q.item_end[w]), start = w > 0 ? uniform64(q.item_end[w - 1]) : 0;
    if (end == start || start >= q.capacity) return;                    // nothing owned, or everything past the list's end
    int64_t ox, y, z;
    uint64_t row;
    const uint64_t faces = brick_faces(q, w, lane, ox, y, z, row);
    // the lane's place: the exclusive scan of the lane counts (lane = y + 8 z: z, then y; inside the lane x, then d)
    const int mine = __popcll(faces);
    int before = mine;
    for (int o = 1; o < 64; o <<= 1) {
        const int v = __shfl_up(before, o);
        if (lane >= o) before += v;
    }
    int64_t at = start + (before - mine);
    // (an entry as ONE 16-byte store where the list is 16-byte aligned was measured and gained nothing: 1.310 against 1.291 ms on
    // the 18.3 M faces of profiles/r15_face_extract_rate.txt; the pass is bound by forming the masks again)
    for (int k = 0; k < kBrick && at < q.capacity; k++) {
        const int material = (int)(row >> (8 * k)) & 0xff;
#pragma unroll
        for (int d = 0; d < 6; d++) {
            if (((faces >> (8 * d + k)) & 1ULL) && at < q.capacity) {
                int32_t *f = q.faces + 4 * at;
                f[0] = (int32_t)(ox + k); f[1] = (int32_t)y; f[2] = (int32_t)z; f[3] = d | (material << 8);
            }
            at += (int64_t)((faces >> (8 * d + k)) & 1ULL);
        }
    }
}

namespace {
// one wave per item; past 2^22 blocks the grid's other two dimensions carry the rest (launch_voxel_regions)
bool face_grid(const FaceParams &q, dim3 &grid) {
    const int64_t waves = q.n * q.bricks[0] * q.bricks[1] * q.bricks[2], blocks = (waves + kFaceThreads / 64 - 1) / (kFaceThreads / 64);
    const int64_t gx = blocks < (1 << 22) ? blocks : (1 << 22), rows = (blocks + gx - 1) / gx;
    const int64_t gy = rows < 65535 ? rows : 65535, gz = (rows + gy - 1) / gy;
    grid = dim3((unsigned)gx, (unsigned)gy, (unsigned)gz);
    return gz <= 65535;
}
}  // namespace

hipError_t launch_face_count(const FaceParams &q, hipStream_t stream) {
    (void)hipGetLastError();
    dim3 grid;
    if (!face_grid(q, grid)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(face_count_kernel, grid, dim3(kFaceThreads), 0, stream, q);
    return hipGetLastError();
}

hipError_t launch_face_regions(const FaceParams &q, hipStream_t stream) {
    (void)hipGetLastError();
    hipLaunchKernelGGL(face_region_kernel, dim3((unsigned)((q.n + kFaceThreads - 1) / kFaceThreads)), dim3(kFaceThreads), 0, stream, q);
    return hipGetLastError();
}

hipError_t launch_face_emit(const FaceParams &q, hipStream_t stream) {
    (void)hipGetLastError();
    dim3 grid;
    if (!face_grid(q, grid)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(face_emit_kernel, grid, dim3(kFaceThreads), 0, stream, q);
    return hipGetLastError();
}

}  // namespace vrc

VRC_AUDIT_TU(faces)
