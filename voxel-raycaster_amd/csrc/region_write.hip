// region_write.hip -- fill boxes and paste dense blocks into the resident scene (vrc_fill_boxes / vrc_write_regions and their
// _device variants, include/vrc.h) for gfx950.
//
// No voxel is ever enumerated.  An operation is six integers (and a material, or a block of bytes); the front end turns the batch
// into (brick, operation) pairs, the edit's stable sort (voxel_edit.hip's edit_sort) leaves every brick's run of operations in
// ascending operation order, and one wave per touched brick applies its run to the brick it holds in registers.  From there on
// the tree branch IS the voxel edit: the same subtree emission (voxel_edit_emit.hpp), the same ancestor pass, the same commit.
//
//   region_write_count_kernel      one lane per operation: clip it to the scene in 64 bits, count the map-aligned 8^3 bricks it
//                                  overlaps (0: the operation is skipped), note whether a fill brings a material other than 0 / 5
//   region_write_materials_kernel  pastes into a tree without attachments: one lane per row of a block, the same question for the
//                                  bytes of its in-scene part
//   (exclusive scan of the counts: rocprim; the host reads the total)
//   region_write_emit_kernel       one wave per operation: the pairs (brick key, operation) at offsets[op] + local
//   shape_write_count_kernel       balls and axis-aligned cylinders (vrc_fill_shapes), one wave per operation: the lanes stride over the
//   shape_write_emit_kernel        brick rows of the clipped bounding box, and the bricks of a row are a closed form (shape_span.hpp) --
//                                  the exact set of bricks that hold a voxel of the shape.  The brick pass below takes each row's x range
//                                  from the same closed form; everything else is the fills'.
//   (sort by key; the unique keys in order: voxel_edit.hip)
//   region_write_brick_kernel      tree, one wave per touched brick: lane = row (y, z), its 8 materials in one 64-bit register.
//                                  The wave walks the run in order -- a wave-uniform loop, the operation's integers are uniform
//                                  loads -- and every lane merges the bytes of its row the operation covers: a byte mask from the
//                                  clipped x range, zeroed where y or z is outside, narrowed by WHERE_EMPTY / WHERE_SOLID (zero-byte
//                                  detection on the row as it is at that moment) and by SKIP_ZERO (on the source bytes).  No LDS
//                                  atomics, no owner table; the rows go to LDS once, for the emission.
//   region_write_map_kernel        map, one wave per touched brick of the map: loads the rows that exist, applies the run, stores
//                                  the bytes that changed
#include <hip/hip_runtime.h>

#include <rocprim/device/device_scan.hpp>

#include "region_write.h"
#include "shape_span.hpp"
#include "svo_node.hpp"
#include "voxel_edit_emit.hpp"
#include "vrc_launch.h"

namespace vrc {

namespace {

// Operation i: its box [lo, hi) in 64 bits (lo + size never wraps) and its material.  false: an operation the _device fill
// could not be refused for (a size below 1, a material outside int8) -- it is skipped.
__device__ inline bool region_op(const RegionParams &p, int64_t i, int64_t lo[3], int64_t hi[3], int &m) {
    bool ok = true;
    m = 0;
    if (p.mode == kRegionPaste) {
        for (int a = 0; a < 3; a++) { lo[a] = p.boxes[3 * i + a]; hi[a] = lo[a] + p.size[a]; }
    } else {
        for (int a = 0; a < 3; a++) {
            const int32_t s = p.boxes[6 * i + 3 + a];
            lo[a] = p.boxes[6 * i + a]; hi[a] = lo[a] + s;
            ok = ok && s >= 1;
        }
        m = p.materials[i];
        ok = ok && m >= -128 && m <= 127;
    }
    return ok;
}

// the bricks [b0, b0 + nb) the in-scene part of [lo, hi) overlaps; false when it is empty
__device__ inline bool region_bricks(const RegionParams &p, const int64_t lo[3], const int64_t hi[3], int64_t b0[3], int64_t nb[3]) {
    bool any = true;
    for (int a = 0; a < 3; a++) {
        const int64_t clo = lo[a] > 0 ? lo[a] : 0, chi = hi[a] < p.lim[a] ? hi[a] : p.lim[a];
        any = any && clo < chi;
        b0[a] = clo >> kReadBrickLog2;
        nb[a] = ((chi - 1) >> kReadBrickLog2) - b0[a] + 1;
    }
    return any;
}

// Shape i as the caller's six integers, and its material
__device__ inline ShapeOp shape_op(const RegionParams &p, int64_t i, int &m) {
    const int32_t *s = p.boxes + 6 * i;
    m = p.materials[i];
    return ShapeOp{s[0], {s[1], s[2], s[3]}, s[4], s[5]};
}

// The brick rows (by, bz) of the shape's bounding box, clipped to the scene in 64 bits: b0[1], b0[2] and nb[1], nb[2] (nb[0], b0[0]
// are not used).  false: the box misses the scene, or the operation is one the _device call could not be refused for.
__device__ inline bool shape_brick_rows(const RegionParams &p, const ShapeOp &s, int m, int64_t b0[3], int64_t nb[3]) {
    if (!shape_valid(s, m)) return false;
    int64_t lo[3], hi[3];
    for (int a = 0; a < 3; a++) {
        const ShapeSpan e = shape_extent(s, a);
        lo[a] = e.a; hi[a] = e.b;
    }
    return region_bricks(p, lo, hi, b0, nb);
}

__device__ inline uint64_t low_bytes(int k) { return k >= 8 ? ~0ULL : (1ULL << (8 * k)) - 1ULL; }

// 0xff in every byte of v that is zero
__device__ inline uint64_t zero_bytes(uint64_t v) {
    constexpr uint64_t k7f = 0x7f7f7f7f7f7f7f7fULL;
    const uint64_t t = ~(((v & k7f) + k7f) | v | k7f);              // 0x80 where the byte is zero
    return (t >> 7) * 0xffULL;
}

// The run [first, last) of the sorted pairs applied, in order, to row (gy, gz) of the brick whose lowest x is ox: `row` holds the
// row's 8 materials, byte k = voxel ox + k.  first and last are wave-uniform.
__device__ inline uint64_t region_apply_run(const RegionParams &p, int64_t first, int64_t last, int ox, int gy, int gz, uint64_t row) {
    for (int64_t i = first; i < last; i++) {
        const int64_t op = p.edit.sorted_order[i];
        int64_t lo[3], hi[3];
        int m;
        bool yz;                                                    // the row is one of the operation's
        if (p.mode == kRegionShapes) {
            // the row's own x range from the closed form (per-lane 64-bit integer work, no branch on it); an empty span: not a row of the shape
            const ShapeSpan x = shape_row_span(shape_op(p, op, m), gy, gz);
            lo[0] = x.a; hi[0] = x.b;
            lo[1] = lo[2] = hi[1] = hi[2] = 0;
            yz = x.a < x.b;
        } else {
            (void)region_op(p, op, lo, hi, m);
            yz = gy >= lo[1] && gy < hi[1] && gz >= lo[2] && gz < hi[2];
        }
        const int64_t xe = hi[0] < p.lim[0] ? hi[0] : p.lim[0];
        const int64_t a64 = lo[0] - ox, b64 = xe - ox;
        const int a = a64 < 0 ? 0 : (a64 > 8 ? 8 : (int)a64), b = b64 < 0 ? 0 : (b64 > 8 ? 8 : (int)b64);
        const bool in = a < b && yz && gy < p.lim[1] && gz < p.lim[2];
        uint64_t mask = in ? low_bytes(b) & ~low_bytes(a) : 0ULL;
        uint64_t val = 0x0101010101010101ULL * (uint64_t)(uint8_t)m;
        if (p.mode == kRegionPaste) {
            val = 0;
            if (mask) {
                // the row's bytes of block `op`, at whatever alignment the block has
                const uint64_t at = (uint64_t)op * p.volume + (uint64_t)((int64_t)ox - lo[0])
                                    + (uint64_t)p.size[0] * ((uint64_t)(gy - lo[1]) + (uint64_t)p.size[1] * (uint64_t)(gz - lo[2]));
                for (int k = a; k < b; k++) val |= (uint64_t)(uint8_t)p.data[at + (uint64_t)k] << (8 * k);
            }
            if (p.flags & kWriteSkipZero) mask &= ~zero_bytes(val);
        }
        if (p.flags & kWriteWhereEmpty) mask &= zero_bytes(row);
        if (p.flags & kWriteWhereSolid) mask &= ~zero_bytes(row);
        row = (row & ~mask) | (val & mask);
    }
    return row;
}

unsigned region_grid_for(int64_t threads) {
    const int64_t blocks = (threads + kEditThreads - 1) / kEditThreads;
    return (unsigned)(blocks < 1 ? 1 : (blocks < (1 << 20) ? blocks : (1 << 20)));   // (larger batches: the lanes loop)
}

}  // namespace

__global__ __launch_bounds__(kEditThreads) void region_write_count_kernel(const RegionParams p) {
    const int64_t stride = (int64_t)gridDim.x * kEditThreads;
    for (int64_t i = (int64_t)blockIdx.x * kEditThreads + threadIdx.x; i <= p.n; i += stride) {
        uint64_t count = 0;
        if (i < p.n) {
            int64_t lo[3], hi[3], b0[3], nb[3];
            int m;
            if (region_op(p, i, lo, hi, m) && region_bricks(p, lo, hi, b0, nb)) {
                count = (uint64_t)nb[0] * (uint64_t)nb[1] * (uint64_t)nb[2];      // (at most 2^21 bricks per axis: 63 bits)
                if (count > (1ULL << 32)) count = 1ULL << 32;                    // (the sum stays below 2^63; the host refuses above 2^31 - 1)
                if (p.edit.scene.svo && p.mode == kRegionFill && m != 0 && m != 5) atomicOr(&p.edit.counters[kEditMaterials], 1ULL);
            } else {
                atomicAdd(&p.edit.counters[kEditSkipped], 1ULL);
            }
        }
        p.counts[i] = count;
    }
}

__global__ __launch_bounds__(kEditThreads) void region_write_materials_kernel(const RegionParams p) {
    const int64_t rows_per = (int64_t)p.size[1] * p.size[2], rows = p.n * rows_per;
    const int64_t stride = (int64_t)gridDim.x * kEditThreads;
    for (int64_t r = (int64_t)blockIdx.x * kEditThreads + threadIdx.x; r < rows; r += stride) {
        const int64_t op = r / rows_per, yz = r % rows_per;
        const int64_t lx = p.boxes[3 * op], gy = (int64_t)p.boxes[3 * op + 1] + yz % p.size[1], gz = (int64_t)p.boxes[3 * op + 2] + yz / p.size[1];
        if (gy < 0 || gy >= p.lim[1] || gz < 0 || gz >= p.lim[2]) continue;
        const int64_t xs = (lx > 0 ? lx : 0) - lx, xe = (lx + p.size[0] < p.lim[0] ? lx + p.size[0] : p.lim[0]) - lx;
        const int8_t *src = p.data + (uint64_t)op * p.volume + (uint64_t)yz * (uint64_t)p.size[0];
        bool other = false;
        for (int64_t k = xs; k < xe; k++) other = other || (src[k] != 0 && src[k] != 5);
        if (other) atomicOr(&p.edit.counters[kEditMaterials], 1ULL);
    }
}

__global__ __launch_bounds__(kEditThreads) void region_write_emit_kernel(const RegionParams p) {
    const int lane = threadIdx.x & 63;
    const int64_t waves = (int64_t)gridDim.x * (kEditThreads / 64);
    for (int64_t op = (int64_t)blockIdx.x * (kEditThreads / 64) + (threadIdx.x >> 6); op < p.n; op += waves) {
        const uint64_t count = p.counts[op], at = p.offsets[op];
        if (!count) continue;
        int64_t lo[3], hi[3], b0[3], nb[3];
        int m;
        (void)region_op(p, op, lo, hi, m);
        (void)region_bricks(p, lo, hi, b0, nb);
        for (uint64_t l = (uint64_t)lane; l < count; l += 64) {
            const uint64_t bx = (uint64_t)b0[0] + l % (uint64_t)nb[0], by = (uint64_t)b0[1] + (l / (uint64_t)nb[0]) % (uint64_t)nb[1],
                           bz = (uint64_t)b0[2] + l / ((uint64_t)nb[0] * (uint64_t)nb[1]);
            p.edit.keys[at + l] = p.edit.scene.svo ? spread3(bx) | (spread3(by) << 1) | (spread3(bz) << 2)
                                                   : bx + (uint64_t)p.nb[0] * (by + (uint64_t)p.nb[1] * bz);
            p.edit.order[at + l] = (uint32_t)op;
        }
    }
}

// Shapes, one wave per operation (operation n: the scan's closing zero).  The lanes stride over the brick rows (by, bz) of the
// shape's clipped bounding box -- so a radius of 2^30 in a 64^3 scene is 8 x 8 rows -- and each row's bricks come from the closed
// form (shape_span.hpp): the count is the exact number of bricks that hold a voxel of the shape, not the box's.
__global__ __launch_bounds__(kEditThreads) void shape_write_count_kernel(const RegionParams p) {
    const int lane = threadIdx.x & 63;
    const int64_t waves = (int64_t)gridDim.x * (kEditThreads / 64);
    for (int64_t op = (int64_t)blockIdx.x * (kEditThreads / 64) + (threadIdx.x >> 6); op <= p.n; op += waves) {
        uint64_t count = 0;
        if (op < p.n) {
            int m;
            const ShapeOp s = shape_op(p, op, m);
            int64_t b0[3], nb[3];
            if (shape_brick_rows(p, s, m, b0, nb)) {
                const uint64_t rows = (uint64_t)nb[1] * (uint64_t)nb[2];
                for (uint64_t l = (uint64_t)lane; l < rows; l += 64) {
                    const ShapeSpan b = shape_brick_row(s, b0[1] + (int64_t)(l % (uint64_t)nb[1]), b0[2] + (int64_t)(l / (uint64_t)nb[1]), p.lim, kReadBrickLog2);
                    count += (uint64_t)(b.b - b.a);
                    if (count > (1ULL << 32)) count = 1ULL << 32;                // (as the boxes': the host refuses above 2^31 - 1)
                }
                for (int d = 32; d >= 1; d >>= 1) count += __shfl_down(count, d, 64);
                count = __shfl(count, 0, 64);
                if (count > (1ULL << 32)) count = 1ULL << 32;
            }
            if (lane == 0) {
                if (!count) atomicAdd(&p.edit.counters[kEditSkipped], 1ULL);
                else if (p.edit.scene.svo && m != 0 && m != 5) atomicOr(&p.edit.counters[kEditMaterials], 1ULL);
            }
        }
        if (lane == 0) p.counts[op] = count;
    }
}

// The same stride; every round takes a wave-wide exclusive prefix of the lanes' interval lengths on top of a running base, and a
// lane writes its row's bricks there.  The order of the pairs inside one operation is free: the stable sort needs the operations
// ascending, and offsets[] gives that.
__global__ __launch_bounds__(kEditThreads) void shape_write_emit_kernel(const RegionParams p) {
    const int lane = threadIdx.x & 63;
    const int64_t waves = (int64_t)gridDim.x * (kEditThreads / 64);
    for (int64_t op = (int64_t)blockIdx.x * (kEditThreads / 64) + (threadIdx.x >> 6); op < p.n; op += waves) {
        const uint64_t count = p.counts[op], at = p.offsets[op];
        if (!count) continue;
        int m;
        const ShapeOp s = shape_op(p, op, m);
        int64_t b0[3], nb[3];
        (void)shape_brick_rows(p, s, m, b0, nb);
        const uint64_t rows = (uint64_t)nb[1] * (uint64_t)nb[2];
        uint64_t base = 0;
        for (uint64_t first = 0; first < rows; first += 64) {      // (every lane takes every round: the prefix is the wave's)
            const uint64_t l = first + (uint64_t)lane;
            const uint64_t by = (uint64_t)b0[1] + l % (uint64_t)nb[1], bz = (uint64_t)b0[2] + l / (uint64_t)nb[1];
            ShapeSpan b = {0, 0};
            if (l < rows) b = shape_brick_row(s, (int64_t)by, (int64_t)bz, p.lim, kReadBrickLog2);
            const uint64_t len = (uint64_t)(b.b - b.a);
            uint64_t upto = len;                                    // inclusive prefix
            for (int d = 1; d < 64; d <<= 1) {
                const uint64_t below = __shfl_up(upto, d, 64);
                if (lane >= d) upto += below;
            }
            const uint64_t local = base + upto - len;
            for (uint64_t j = 0; j < len && local + j < count; j++) {            // (never past the operation's own pairs)
                const uint64_t bx = (uint64_t)b.a + j;
                p.edit.keys[at + local + j] = p.edit.scene.svo ? spread3(bx) | (spread3(by) << 1) | (spread3(bz) << 2)
                                                               : bx + (uint64_t)p.nb[0] * (by + (uint64_t)p.nb[1] * bz);
                p.edit.order[at + local + j] = (uint32_t)op;
            }
            base += __shfl(upto, 63, 64);
        }
    }
}

// shallow: as voxel_edit_brick_kernel's
__global__ __launch_bounds__(kEditThreads) void region_write_brick_kernel(const RegionParams p, const int shallow) {
    constexpr int kWaves = kEditThreads / 64;
    __shared__ uint64_t s_rows[kWaves][64];                        // the new brick, for the emission: row (y, z) = lane, byte x
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63, ly = lane & 7, lz = lane >> 3;
    const int64_t u = (int64_t)blockIdx.x * kWaves + wave;         // (wave-uniform: the run's loads are scalar)
    const bool live = u < p.edit.n_bricks;                         // (no early exit: the block's barrier is taken by every wave)
    uint64_t old_row = 0, row = 0;
    if (live) {
        const uint64_t key = p.edit.brick_keys[u];
        old_row = edit_old_row(p.edit, key, ly, lz);
        const int64_t first = lower_bound(p.edit.sorted_keys, p.edit.n, key), last = lower_bound(p.edit.sorted_keys, p.edit.n, key + 1);
        const int ox = (int)(compact3(key) << kReadBrickLog2), oy = (int)(compact3(key >> 1) << kReadBrickLog2), oz = (int)(compact3(key >> 2) << kReadBrickLog2);
        row = region_apply_run(p, first, last, ox, oy + ly, oz + lz, old_row);
    }
    s_rows[wave][lane] = row;
    __syncthreads();
    edit_emit_brick(p.edit, shallow, u, lane, live, old_row, s_rows[wave]);
}

__global__ __launch_bounds__(kEditThreads) void region_write_map_kernel(const RegionParams p) {
    constexpr int kWaves = kEditThreads / 64;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63, ly = lane & 7, lz = lane >> 3;
    const int64_t u = (int64_t)blockIdx.x * kWaves + wave;
    if (u >= p.edit.n_bricks) return;
    const uint64_t key = p.edit.brick_keys[u];
    const int ox = (int)(key % (uint64_t)p.nb[0]) << kReadBrickLog2, gy = ((int)((key / (uint64_t)p.nb[0]) % (uint64_t)p.nb[1]) << kReadBrickLog2) + ly,
              gz = ((int)(key / ((uint64_t)p.nb[0] * (uint64_t)p.nb[1])) << kReadBrickLog2) + lz;
    const int nx = p.lim[0] - ox < 8 ? p.lim[0] - ox : 8;         // x clipped at dx
    // the frame's index of the row's first voxel; a row outside map_dim or past the array is left alone
    const uint64_t base = (uint64_t)ox + (uint64_t)p.edit.scene.map_dim[0] * ((uint64_t)gy + (uint64_t)p.edit.scene.map_dim[2] * (uint64_t)gz);
    const bool exists = gy < p.lim[1] && gz < p.lim[2] && base + (uint64_t)nx <= p.edit.scene.map_bytes;
    uint64_t old_row = 0;
    if (exists)
        for (int k = 0; k < nx; k++) old_row |= (uint64_t)(uint8_t)p.edit.map[VRC_IDX(kMap, base + (uint64_t)k)] << (8 * k);
    const int64_t first = lower_bound(p.edit.sorted_keys, p.edit.n, key), last = lower_bound(p.edit.sorted_keys, p.edit.n, key + 1);
    const uint64_t row = region_apply_run(p, first, last, ox, gy, gz, old_row);
    int changed = 0;
    if (exists) {
        const uint64_t diff = old_row ^ row;
        for (int k = 0; k < nx; k++)
            if ((diff >> (8 * k)) & 0xffULL) {
                p.edit.map[VRC_IDX(kMap, base + (uint64_t)k)] = (int8_t)(row >> (8 * k));
                changed++;
            }
    }
    for (int d = 32; d >= 1; d >>= 1) changed += __shfl_down(changed, d, 64);
    if (lane == 0 && changed) atomicAdd(&p.edit.counters[kEditChanged], (unsigned long long)changed);
}

hipError_t launch_region_count(const RegionParams &p, hipStream_t stream) {
    (void)hipGetLastError();
    hipLaunchKernelGGL(region_write_count_kernel, dim3(region_grid_for(p.n + 1)), dim3(kEditThreads), 0, stream, p);
    return hipGetLastError();
}

hipError_t launch_region_materials(const RegionParams &p, hipStream_t stream) {
    (void)hipGetLastError();
    hipLaunchKernelGGL(region_write_materials_kernel, dim3(region_grid_for(p.n * p.size[1] * p.size[2])), dim3(kEditThreads), 0, stream, p);
    return hipGetLastError();
}

// exclusive scan of n 64-bit counts; temp == nullptr: *temp_bytes receives the storage needed
hipError_t region_scan(void *temp, size_t *temp_bytes, const uint64_t *in, uint64_t *out, int64_t n, hipStream_t stream) {
    return rocprim::exclusive_scan(temp, *temp_bytes, in, out, (uint64_t)0, (size_t)n, rocprim::plus<uint64_t>(), stream);
}

hipError_t launch_region_emit(const RegionParams &p, hipStream_t stream) {
    (void)hipGetLastError();
    hipLaunchKernelGGL(region_write_emit_kernel, dim3(region_grid_for(p.n * 64)), dim3(kEditThreads), 0, stream, p);
    return hipGetLastError();
}

hipError_t launch_shape_count(const RegionParams &p, hipStream_t stream) {
    (void)hipGetLastError();
    hipLaunchKernelGGL(shape_write_count_kernel, dim3(region_grid_for((p.n + 1) * 64)), dim3(kEditThreads), 0, stream, p);
    return hipGetLastError();
}

hipError_t launch_shape_emit(const RegionParams &p, hipStream_t stream) {
    (void)hipGetLastError();
    hipLaunchKernelGGL(shape_write_emit_kernel, dim3(region_grid_for(p.n * 64)), dim3(kEditThreads), 0, stream, p);
    return hipGetLastError();
}

hipError_t launch_region_bricks(const RegionParams &p, hipStream_t stream) {
    (void)hipGetLastError();
    const int64_t blocks = (p.edit.n_bricks + kEditThreads / 64 - 1) / (kEditThreads / 64);
    if (blocks < 1 || blocks > 0x7fffffffLL) return hipErrorInvalidValue;
    if (p.edit.scene.svo)
        hipLaunchKernelGGL(region_write_brick_kernel, dim3((unsigned)blocks), dim3(kEditThreads), 0, stream, p,
                           p.edit.scene.log2_dim <= kReadBrickLog2 ? p.edit.scene.log2_dim : 0);
    else
        hipLaunchKernelGGL(region_write_map_kernel, dim3((unsigned)blocks), dim3(kEditThreads), 0, stream, p);
    return hipGetLastError();
}

}  // namespace vrc

VRC_AUDIT_TU(region)
