// Everything the host layer (vrc_api.cpp, vrc_query.cpp, vrc_scene_edit.cpp) calls in the .hip files: the kernel launchers and the device builders.  Included by
// them and by every file that defines one of these functions, so the compiler holds each definition against its
// declaration.  The argument blocks themselves live in vrc_params.h, raycast_query.h, box_query.h, box_sweep.h, voxel_read.h, face_extract.h, voxel_edit.h, region_write.h and octree_compact.h.
#pragma once

#include <hip/hip_runtime.h>

#include <stdint.h>

#include <string>

#include "../../include/vrc.h"

namespace vrc {

struct RaycastParams;
struct LaunchRecord;
struct QueryParams;
struct BoxParams;
struct SweepParams;
struct ReadParams;
struct FaceParams;
struct EditParams;
struct EditLevel;
struct RegionParams;
struct CompactParams;
struct CompactLevel;

// raycast_kernel.hip
hipError_t launch_fill_image(float *image, size_t n_pixels, hipStream_t stream);
hipError_t launch_pack_rgba8(const float *image, uint8_t *out, size_t n_pixels, hipStream_t stream);
hipError_t launch_frame_setup(const RaycastParams &p, hipStream_t stream);
int jump_tables_lds_rows(const RaycastParams &p);
int raycast_workgroup_tiles(const RaycastParams &p);
int raycast_workgroups(const RaycastParams &p);
hipError_t launch_raycast(const RaycastParams &p, hipStream_t stream, LaunchRecord *rec);
hipError_t launch_reduce_counters(const unsigned long long *partials, int nblocks, unsigned long long *out,
                                  hipStream_t stream);

// raycast_jump_kernel.hip
hipError_t launch_raycast_jump(const RaycastParams &p, hipStream_t stream, LaunchRecord *rec);
hipError_t launch_coarse_build(const uint64_t *descriptors, uint64_t root_index, int log2_dim, int lc, uint64_t *out, hipStream_t stream);

// empty_boxes.hip
hipError_t launch_box_positions(const uint64_t *descriptors, uint64_t n_desc, uint64_t root_index, int n, uint64_t *pos, hipStream_t stream);
hipError_t launch_box_build(const uint64_t *descriptors, uint64_t n_desc, uint64_t root_index, int n, int lc, uint64_t *pos_tmp,
                            uint32_t *boxes, uint32_t *aux, hipStream_t stream);
// What launch_box_build_upper leaves behind (device memory, the caller frees it): records 0 .. count-1 for the descriptors of the
// levels 0 .. levels-1.
struct BoxUpper { uint64_t *desc = nullptr, *pos = nullptr; uint32_t *child = nullptr, *boxes = nullptr; uint64_t count = 0; int levels = 0; };
hipError_t launch_box_build_upper(const uint64_t *descriptors, uint64_t root_index, int n, int lc, uint64_t max_records, int max_levels,
                                  BoxUpper *out, uint32_t *aux, hipStream_t stream);
hipError_t box_queries_cut(unsigned long long *out);
hipError_t launch_box_check_cells(const uint64_t *descriptors, uint64_t root_index, int n, int lc, const uint32_t *aux, uint64_t samples,
                                  uint64_t seed, unsigned long long *result, hipStream_t stream);
hipError_t launch_box_check(const uint64_t *descriptors, uint64_t n_records, uint64_t root_index, int n, const uint64_t *pos, const uint64_t *desc_of,
                            const uint32_t *boxes, uint64_t samples, uint64_t seed, unsigned long long *result, hipStream_t stream);

// raycast_query.hip
hipError_t launch_raycast_query(const QueryParams &q, hipStream_t stream);

// box_query.hip
hipError_t launch_box_plan(const BoxParams &q, int64_t *small_cnt, int64_t *big_cnt, hipStream_t stream);
hipError_t launch_box_count(const BoxParams &q, int pass, hipStream_t stream);
hipError_t launch_box_finalize(const BoxParams &q, hipStream_t stream);
hipError_t box_scan(void *temp, size_t *temp_bytes, const int64_t *in, int64_t *out, int64_t n, hipStream_t stream);

// box_sweep.hip
hipError_t launch_sweep_plan(const SweepParams &p, int64_t *big_cnt, hipStream_t stream);
hipError_t launch_sweep(const SweepParams &p, hipStream_t stream);

// voxel_read.hip
hipError_t launch_voxel_points(const ReadParams &q, hipStream_t stream);
hipError_t launch_voxel_regions(const ReadParams &q, hipStream_t stream);

// face_extract.hip
hipError_t launch_face_count(const FaceParams &q, hipStream_t stream);
hipError_t launch_face_regions(const FaceParams &q, hipStream_t stream);
hipError_t launch_face_emit(const FaceParams &q, hipStream_t stream);

// voxel_edit.hip
hipError_t launch_edit_keys(const EditParams &q, hipStream_t stream);
hipError_t edit_sort(void *temp, size_t *temp_bytes, const uint64_t *keys_in, uint64_t *keys_out, const uint32_t *order_in, uint32_t *order_out,
                     int64_t n, int bits, hipStream_t stream);
hipError_t edit_runs(void *temp, size_t *temp_bytes, const uint64_t *sorted_keys, int64_t n, uint64_t *unique, uint32_t *counts,
                     unsigned long long *n_runs, hipStream_t stream);
hipError_t launch_edit_array(const EditParams &q, hipStream_t stream);
hipError_t launch_edit_bricks(const EditParams &q, hipStream_t stream);
hipError_t launch_edit_level(const EditParams &q, const EditLevel &level, hipStream_t stream);

// region_write.hip
hipError_t launch_region_count(const RegionParams &p, hipStream_t stream);
hipError_t launch_region_materials(const RegionParams &p, hipStream_t stream);
hipError_t region_scan(void *temp, size_t *temp_bytes, const uint64_t *in, uint64_t *out, int64_t n, hipStream_t stream);
hipError_t launch_region_emit(const RegionParams &p, hipStream_t stream);
hipError_t launch_shape_count(const RegionParams &p, hipStream_t stream);
hipError_t launch_shape_emit(const RegionParams &p, hipStream_t stream);
hipError_t launch_region_bricks(const RegionParams &p, hipStream_t stream);

// octree_compact.hip
hipError_t launch_compact_level(const CompactParams &q, const CompactLevel &level, int pass, hipStream_t stream);
hipError_t launch_compact_root(const CompactParams &q, hipStream_t stream);
hipError_t launch_compact_materials(const CompactParams &q, const uint64_t *remap, uint64_t n_new, uint64_t *attach, uint64_t n_attach_new, hipStream_t stream);
hipError_t compact_scan(void *temp, size_t *temp_bytes, const uint64_t *in, uint64_t *out, uint64_t n, hipStream_t stream);

// svo_builder_gpu.hip
int build_shell_terrain_device(hipStream_t stream, uint32_t depth, uint64_t seed, int32_t thickness, int32_t octave_floor,
                               uint32_t flags, uint64_t validate_samples, const int32_t *probe_xy, uint32_t n_probe,
                               int32_t *probe_lohi, uint64_t **d_desc, vrc_build_info *out, std::string &error);
int build_columns_device(hipStream_t stream, uint32_t depth, uint64_t seed, int32_t thickness, int32_t octave_floor,
                         const uint16_t *host_hi, const uint16_t *host_lo,
                         uint32_t flags, uint64_t validate_samples, const int32_t *probe_xy, uint32_t n_probe,
                         int32_t *probe_lohi, uint64_t **d_desc, vrc_build_info *out, std::string &error);
int build_grid_device(hipStream_t stream, uint32_t depth, const int8_t *host_grid, const int8_t *resident_grid, uint32_t flags,
                      uint64_t validate_samples, uint64_t **d_desc, uint32_t **d_lookup, uint64_t **d_attach, uint64_t *n_attach,
                      vrc_build_info *out, std::string &error);

}  // namespace vrc
