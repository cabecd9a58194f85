/*
 * vrc.h -- C ABI of the MI355X-native raycast path ("libvrc.so").
 *
 * Drop-in boundary for the reference's CLCaster subsystem
 * (include/CLCaster.h:93-329, src/CLCaster.cpp).  Every entry point names the
 * reference interface it replaces.  Plain pointers and sizes only; no C++,
 * torch, OpenCL or GL types cross this boundary.
 *
 * Conventions
 *   - every function returns a vrc_status (0 = ok); the reference returns
 *     bool and logs through Logger (CLCaster.cpp:1011-1017).  Details of the
 *     last failure: vrc_last_error().  Nothing aborts or throws.
 *   - scene buffers are COPIED at call time (reference: CL_MEM_COPY_HOST_PTR,
 *     CLCaster.cpp:893-896); camera, lights and light_count are RETAINED
 *     pointers re-read on every vrc_compute (reference: CL_MEM_USE_HOST_PTR,
 *     CLCaster.cpp:137-139,322) -- the caller keeps them alive.
 *   - a handle is not thread-safe (the reference is single-threaded, SURVEY
 *     8b): one host thread at a time per handle.  DIFFERENT handles may be
 *     driven from different host threads, also when they hold one tree
 *     (vrc_assign_octree_from): what is derived from a tree is built once under
 *     the tree's guard, and a frame holds that guard from the moment it reads
 *     the tree's pointers until its kernel is enqueued.  Holders of one tree
 *     should agree on octree_root_index, octree_dimensions and coarse_log2: if
 *     they differ every frame rebuilds the table and the boxes for ITS settings
 *     (correct, but 0.6 s per frame at depth 12).
 *     A handle from vrc_create drives ONE GPU; multi-GPU is either one
 *     such handle per GPU and process, each rendering its own row slice
 *     (vrc_set_row_slice), or ONE group handle from vrc_create_group that
 *     drives n GPUs from one host thread -- the reference's single synchronous
 *     compute() (CLCaster.cpp:224-228,946-987) spread over the row bands of n
 *     devices.  No collective either way: the SVO is replicated, tiles are
 *     copied out by the GPU that rendered them.
 *   - the GL-shared output texture of the reference (CLCaster.cpp:278-296) is
 *     replaced by an offline float4 pixel buffer in HBM, read back with
 *     vrc_read_image_*.
 */
#ifndef VRC_H
#define VRC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct vrc_caster vrc_caster;

typedef enum vrc_status {
    VRC_OK = 0,
    VRC_ERR_INVALID_ARGUMENT = 1,
    VRC_ERR_NOT_READY = 2,      /* validate()/compute() before the required assign_* calls */
    VRC_ERR_DEVICE = 3,         /* a HIP call failed; see vrc_last_error */
    VRC_ERR_OUT_OF_MEMORY = 4,
    VRC_ERR_NOT_FOUND = 5,      /* unknown setting name */
    VRC_ERR_LIMIT = 6           /* > 64 settings, octree deeper than the kernel stack, ... */
} vrc_status;

/* ---- lifecycle ------------------------------------------------------- */

/* CLCaster::CLCaster + CLCaster::init (CLCaster.cpp:14-74).  The interactive
 * device prompt / device_config.bin (:23-48,495-542) is replaced by
 * device_ordinal.  Fails with VRC_ERR_DEVICE when no HIP device is present:
 * there is no CPU fallback.                                                  */
int vrc_create(int device_ordinal, vrc_caster **out);
/* CLCaster::~CLCaster (CLCaster.cpp:5-12); unlike the reference this frees all
 * device memory.                                                            */
int vrc_destroy(vrc_caster *h);
/* Logger::log(..., ERROR) + cl_err_lookup (CLCaster.cpp:1112-1310) */
const char *vrc_last_error(const vrc_caster *h);
/* aquire_hardware (CLCaster.cpp:430-493): number of usable GPUs */
int vrc_device_count(int *count);

/* ---- scene buffers (copied) ------------------------------------------- */

/* CLCaster::assign_map (CLCaster.cpp:76-87): "map" char[dx*dy*dz] indexed
 * x + dx*(y + dz*z) by the kernel (ray_caster_kernel.cl:569), "map_dimensions". */
int vrc_assign_map(vrc_caster *h, const int8_t *voxels, int32_t dx, int32_t dy, int32_t dz);
/* CLCaster::release_map (CLCaster.cpp:89-99) */
int vrc_release_map(vrc_caster *h);

/* CLCaster::assign_octree (CLCaster.cpp:102-116): "octree_descriptor_buffer"
 * (n 64-bit child descriptors, format of include/map/Octree.h:89-94) and the
 * "octree_root_index" setting.  The two attachment buffers the reference
 * uploads but never reads (ray_caster_kernel.cl:143-144) are optional.        */
int vrc_assign_octree(vrc_caster *h, const uint64_t *descriptors, uint64_t n_descriptors,
                      uint64_t root_index);
/* Attachment layout (ours; the reference never defined one): lookup[i] (parallel to
 * the descriptor array) = slot in `attachments` of bottom-level descriptor i, whose
 * byte k is the int8 material of child k.  With attachments assigned the SVO branch
 * renders exactly what the array branch renders for the same grid (materials 5 and 6
 * are solid to the renderer, everything else is passed through,
 * ray_caster_kernel.cl:575); without them every valid voxel is material 5.        */
int vrc_assign_octree_attachments(vrc_caster *h, const uint32_t *lookup, uint64_t n_lookup,
                                  const uint64_t *attachments, uint64_t n_attachments);
/* CLCaster::assign_octree for a tree ANOTHER handle on the same GPU already holds (CLCaster.cpp:102-116 uploads the same
 * array again for every caster and never frees it, :5-12): h adopts src's descriptor array, its materials and everything
 * the kernels derive from them (the dense table of the tree's top, the empty boxes) -- they exist once, and live until the
 * last handle that holds them releases them or is destroyed.  Materials assigned later through either handle are seen by
 * both from their next frame on.                                                                                          */
int vrc_assign_octree_from(vrc_caster *h, vrc_caster *src);
/* CLCaster::release_octree (CLCaster.cpp:119-131) */
int vrc_release_octree(vrc_caster *h);

/* CLCaster::create_viewport (CLCaster.cpp:233-299): builds the float4 ray table
 * exactly like the reference (v_fov / h_fov are accepted and ignored, as there)
 * and the output image, initialised to RGBA8 (255,255,255,100).              */
int vrc_create_viewport(vrc_caster *h, int32_t width, int32_t height, float v_fov, float h_fov);
/* Extension: same buffers as vrc_create_viewport but the float4[width*height]
 * ray table ("viewport_matrix", CLCaster.cpp:242-275) is supplied by the host,
 * e.g. a supersampled or differently projected lens.                          */
int vrc_create_viewport_table(vrc_caster *h, int32_t width, int32_t height, const float *table);
/* CLCaster::release_viewport (CLCaster.cpp:301-311) */
int vrc_release_viewport(vrc_caster *h);

/* CLCaster::create_texture_atlas (CLCaster.cpp:208-222): the sf::Texture is
 * replaced by its RGBA8 pixels.                                              */
int vrc_create_texture_atlas(vrc_caster *h, const uint8_t *rgba8, int32_t width, int32_t height,
                             int32_t tile_w, int32_t tile_h);

/* ---- live buffers (retained pointers) --------------------------------- */

/* CLCaster::assign_camera (CLCaster.cpp:133-143): direction = 2 floats
 * (inclination, azimuth), position = 3 floats.                              */
int vrc_assign_camera(vrc_caster *h, const float *direction2, const float *position3);
/* The sin / cos of the two camera angles, supplied by the host: trig4 = { sin(direction.x), cos(direction.x),
 * sin(direction.y), cos(direction.y) }, the four values the reference kernel evaluates per pixel with the OpenCL
 * library's sin / cos (ray_caster_kernel.cl:280-291).  RETAINED like the camera itself and re-read on every
 * vrc_compute; NULL (the default) = the library evaluates sinf / cosf of the live direction on the host once per frame
 * (SURVEY D2).  A host that evaluates them the way its reference build did -- or replays stored values, as
 * tests/test_reference_vectors_gpu.py does with the reference kernel's own -- gets exactly that build's rays: the two
 * libraries' results differ in the last bit for some angles, and one ulp of a direction is another ray table.
 * vrc_release_camera drops the pointer with the camera.                                                              */
int vrc_assign_camera_trig(vrc_caster *h, const float *trig4);
/* CLCaster::release_camera (CLCaster.cpp:145-155) */
int vrc_release_camera(vrc_caster *h);
/* CLCaster::assign_lights (CLCaster.cpp:313-328): packed = 10 floats per light
 * {rgbi[4], position[3], direction[3]} (include/LightController.h:63-73), 8
 * reserved slots in the reference; light_count points at the live count.
 * The reference kernel shades with light 0 only whatever *light_count holds
 * (ray_caster_kernel.cl:264,660-670) and so does this library by default.
 * Extension: setting "light_count" = n > 1 shades with the first
 * min(n, *light_count, 8) lights, each shadow ray restarted from the primary
 * hit ("first-strike resetting", TODO src/main.cpp:33).  */
int vrc_assign_lights(vrc_caster *h, const float *packed, const int32_t *light_count);

/* ---- settings buffer --------------------------------------------------- */

/* CLCaster::add_to_settings_buffer (CLCaster.cpp:1029-1064): appends a slot
 * (max 64, include/CLCaster.h:303).  `define` is the kernel-side macro name the
 * reference passes as -D<define>=<slot>; kept for API fidelity.  Names the
 * kernel understands:
 *   octree_dimensions  (OCTDIM)            required in SVO mode
 *   using_octree       (OCTENABLED)        0 => occupancy from the SVO, != 0 => dense map
 *   octree_root_index  (OCTREE_ROOT_INDEX) set by vrc_assign_octree
 * extensions (defaults reproduce the reference):
 *   max_distance (20: the :325/:357 step cap; |value| <= 2^30, the counter is the reference's int)
 *   shadow_rays (1)  light_count (1, see vrc_assign_lights)
 *   octree_bias (1: the :353-354 term as in the reference; 0: without it)
 *   hit_records (1: the 8 x int32 record per pixel behind vrc_read_hits; 0: none -- the reference has none)
 *   stepping_mode (0: exact per-voxel DDA, bit-identical to the array branch; 1: node-exit jumps, DESIGN.md "mode B")
 *   coarse_log2 (-1: by depth = min(depth - 2, 9) from depth 5, 10 from depth 14; 0: none; k: 2^k cells per axis, at most
 *     min(depth - 2, 10)): the levels of the tree above level k as a dense table in HBM (8 << 3k bytes: 1 GB at k = 9), built on
 *     the device from the descriptor array by vrc_prepare / vrc_validate (or by the first vrc_compute that finds it missing).
 *     Both SVO kernels read it instead of descending from the root; frames, hit records and the exact mode's counters are the same with and without it
 *   empty_boxes (-1: by the tree's size; 0: never -- the canonical traversal, canonical read counts; 1: a box word per descriptor and
 *     child, trees below 2^31 descriptors; 2: box records for the upper levels only -- any tree): an empty node is widened to the
 *     empty box a device-side pass over the descriptor array found around it (vrc_prepare builds the words); frames and hit
 *     records unchanged but for the read count (vrc_counters_canonical).  By default a word per descriptor up to 2^29 descriptors
 *     (32 bytes each), beyond that records for as many upper levels as empty_box_records (default 400 M: 36 bytes each, 52 while
 *     building; at most a quarter of the free device memory) reach; empty_box_levels caps the levels
 *   jump_tables_lds (2: the Euclid tables of the exact closed-form jumps live in LDS when they fit at full occupancy;
 *     1 / 0: always / never)   jump_min_run (closed-form jumps for runs of at least this many iterations; 1 << 24: off)
 * Settings stay live after vrc_validate (overwrite_setting needs no recompile); structural ones are re-checked by
 * every vrc_compute, which fails with an error code instead of launching on a bad value.                            */
int vrc_setting_add(vrc_caster *h, const char *name, const char *define, int64_t value);
/* CLCaster::overwrite_setting (CLCaster.cpp:1087-1109) */
int vrc_setting_set(vrc_caster *h, const char *name, int64_t value);
int vrc_setting_get(vrc_caster *h, const char *name, int64_t *value);

/* ---- validate / compute ------------------------------------------------ */

/* CLCaster::validate (CLCaster.cpp:157-206): checks that camera, map/octree,
 * viewport, lights and atlas are present and consistent.  No runtime
 * compilation happens: the kernels are prebuilt gfx950 code.  Where the
 * reference pays its one-off cost (the kernel build, :157-206) this call pays
 * ours: it ends with vrc_prepare, so the first vrc_compute costs a frame.      */
int vrc_validate(vrc_caster *h);
/* Builds what the SVO kernels derive from the tree for the current settings -- the dense table of the tree's top (setting
 * coarse_log2) and the empty boxes (setting empty_boxes): 15 ms + 0.6 s for the 20 M descriptors of a 4096^3 terrain,
 * 2.6 s at 8192^3, 10 s for the 345 M descriptors of a 16384^3 terrain or the 400 M box records of a deeper one -- so that no
 * frame has to.  Needs the octree and the settings octree_dimensions / using_octree;
 * vrc_validate calls it.  Both structures are optional: a failed allocation is not an error (the frames are rendered by the
 * kernels without them, vrc_memory_usage2().note says why).  A vrc_compute that finds them missing or built for other
 * settings (root, depth, level changed after validate) still builds them itself, synchronously, inside that call -- also
 * vrc_compute_async: it then blocks for the build.                                                                      */
int vrc_prepare(vrc_caster *h);

/* CLCaster::compute (CLCaster.cpp:224-228) -> run_kernel (:946-987).
 * Synchronous like the reference's clFinish (:970).                          */
int vrc_compute(vrc_caster *h);
/* Enqueue one frame on the handle's stream without waiting / wait for it.    */
int vrc_compute_async(vrc_caster *h);
int vrc_sync(vrc_caster *h);

/* Multi-GPU row tiling: this handle renders only the bands
 * b with b % world == rank, a band being `band_rows` consecutive image rows
 * (multiple of 8).  Default rank 0 / world 1 = the whole image.  The buffers
 * stay full-frame (rows of other ranks keep their previous contents).        */
int vrc_set_row_tiling(vrc_caster *h, int32_t rank, int32_t world, int32_t band_rows);
/* Same partition, but the ray table, the frame and the hit records hold ONLY this rank's rows (SURVEY 8e "sliced per
 * GPU: ray table rows and framebuffer rows"): per-rank memory and uploads are 1/world of the frame.  Call before
 * vrc_create_viewport(_table); the read-back calls then fill this rank's rows of the caller's full frame and leave the
 * others alone, so world handles reading into one buffer assemble the frame.                                        */
int vrc_set_row_slice(vrc_caster *h, int32_t rank, int32_t world, int32_t band_rows);

/* One host thread, n GPUs (SURVEY 8b "Compute", 8e): the returned handle is rank 0 of a group of n handles
 * (device_ordinals[r] for rank r; the same ordinal may repeat), row-sliced in bands of band_rows.  Every call on the
 * group handle is replicated on all ranks: the octree is uploaded (or built) once on rank 0's GPU and fanned out
 * device to device (hipMemcpyPeerAsync; ranks on rank 0's own GPU share its arrays), vrc_compute launches every rank
 * and returns when the frame is complete on all of them -- the one synchronous compute() of CLCaster.cpp:224-228,946-987
 * -- vrc_read_* gather every rank's rows into the caller's frame (each GPU copies its own tile, no collective),
 * vrc_get_counters sums the ranks.  vrc_destroy on the group handle destroys all ranks.                            */
int vrc_create_group(const int32_t *device_ordinals, int32_t n, int32_t band_rows, vrc_caster **out);
/* The same with flags.  VRC_GROUP_OWN_COPIES: ranks that sit on rank 0's own GPU do not share its arrays but take the
 * path a rank on another GPU takes -- own allocation, hipMemcpyPeerAsync, attachment re-copy, release -- so that the
 * multi-GPU code can be exercised on a machine with one GPU (vrc_create_group honours VRC_GROUP_OWN_COPIES=1 in the
 * environment).  After a successful creation vrc_last_error() names the ranks whose GPU has no direct peer access to
 * rank 0's (their copies are staged by the runtime); it is empty otherwise.                                          */
#define VRC_GROUP_OWN_COPIES 1u
int vrc_create_group_ex(const int32_t *device_ordinals, int32_t n, int32_t band_rows, uint32_t flags, vrc_caster **out);
int vrc_group_size(const vrc_caster *h, int32_t *n);
/* Pin / unpin a caller-owned frame buffer (hipHostRegister): a group then copies every rank's tile straight into it.
 * A pageable destination works too -- each rank stages its tile through a pinned buffer of its own so that the n copies
 * still run side by side, at the price of one more host copy.                                                        */
int vrc_pin_host_buffer(void *p, size_t bytes);
int vrc_unpin_host_buffer(void *p);
/* Device memory held by one rank of a group (rank 0 = the handle itself). */
typedef struct vrc_memory {
    int32_t  device, rows;            /* GPU ordinal; rows of the frame this rank's buffers hold */
    uint64_t viewport_bytes, image_bytes, hit_bytes, octree_bytes;
    int32_t  octree_shared;           /* 1: the arrays belong to rank 0 (same GPU) */
    int32_t  peer_access;             /* -1: rank 0 or on rank 0's GPU; 1: direct peer access to rank 0's GPU; 0: staged by the runtime */
    uint64_t coarse_bytes;            /* the dense table of the tree's top (setting coarse_log2), 0 before the first frame */
} vrc_memory;
int vrc_memory_usage(vrc_caster *h, int32_t rank, vrc_memory *out);
/* The same with a size-versioned struct: set struct_size = sizeof(vrc_memory2) before the call; the library writes no more
 * than that many bytes and stores how many it wrote, so a host compiled against an older header keeps working when fields
 * are appended.  (vrc_memory grew by coarse_bytes in round 4 without such a field: hosts compiled against the round-3 header
 * must be recompiled or move to this call.)                                                                              */
typedef struct vrc_memory2 {
    uint32_t struct_size;             /* in: sizeof the caller's struct; out: bytes written */
    int32_t  device, rows;
    int32_t  octree_shared;           /* 1: the tree is also held by another handle (group rank on the same GPU, vrc_assign_octree_from) */
    int32_t  peer_access;
    int32_t  tree_holders;            /* handles that hold this rank's tree: its arrays, its coarse table and its boxes exist ONCE */
    int32_t  coarse_log2;             /* level of the dense table of the tree's top, 0: none */
    int32_t  empty_boxes;             /* 1: this rank's last frame was rendered with the tree's empty boxes (setting empty_boxes) */
    uint64_t viewport_bytes, image_bytes, hit_bytes, octree_bytes;
    uint64_t coarse_bytes, box_bytes; /* per TREE, not per handle */
    double   box_build_seconds;
    char     note[160];               /* why an optional structure is missing (allocation failure), else empty */
    uint64_t box_queries_cut;         /* region queries of the boxes' build that gave up at their budget of 4096 descents: the
                                         boxes next to them are smaller than they could be (never wrong); 0 on every BASELINE scene */
    uint64_t box_records;             /* descriptors that carry box words: all of them, or those of the upper box_levels levels */
    int32_t  box_levels, reserved_;   /* levels of the tree (from the root) whose descriptors have box records */
} vrc_memory2;
int vrc_memory_usage2(vrc_caster *h, int32_t rank, vrc_memory2 *out);

/* Self-check of the empty boxes the last frame was rendered with (setting empty_boxes; a derived structure like the coarse
 * table, no counterpart in the reference: Octree.cpp never annotates empty space): `samples` pseudo-random (descriptor,
 * child) pairs are drawn, for each empty child one voxel of its box is looked up in the tree.  *solid_voxels must come back
 * 0.  build_seconds: device time of the boxes' construction.  Any out pointer may be NULL.                              */
int vrc_empty_boxes_check(vrc_caster *h, uint64_t samples, uint64_t seed, uint64_t *boxes_sampled, uint64_t *solid_voxels,
                          double *build_seconds);
/* The box words themselves: out[8 * i + k] belongs to child slot k = x | y<<1 | z<<2 of descriptor first_descriptor + i and
 * means something where that child is empty (not valid): six 5-bit extents, bits 0-4 -x, 5-9 -y, 10-14 -z, 15-19 +x, 20-24 +y,
 * 25-29 +z, in units of the child's own size; code c stands for c (c < 4), (4 | c & 3) << (c / 4 - 1) otherwise.  The box is
 * the child's cube widened by those extents, clamped to the map.  (tests/test_boxes_gpu.py checks every voxel of every box of
 * small trees against the dense grid on the host.)                                                                         */
int vrc_read_empty_boxes(vrc_caster *h, uint64_t first_descriptor, uint64_t count, uint32_t *out);

/* ---- output ------------------------------------------------------------ */

/* CLCaster::draw (CLCaster.cpp:330-332) has no read-back; these replace it.
 * n_floats / n_bytes / n_int32 are the capacities of the caller's buffers.   */
int vrc_read_image_f32(vrc_caster *h, float *rgba, size_t n_floats);
/* What CLCaster::draw shows: the reference's output IS an RGBA8 texture (CLCaster.cpp:278-296,330-332).  The frame is
 * quantised on the device (saturate, x255, round to nearest even, like write_imagef to CL_UNORM_INT8) and 4 bytes per
 * pixel are read back.                                                                                              */
int vrc_read_image_rgba8(vrc_caster *h, uint8_t *rgba, size_t n_bytes);
/* 8 int32 per pixel: voxel x,y,z of the primary hit (-1 if none), material,
 * face bits, flags, final step count, descriptor reads -- SURVEY 8(d)'s canonical
 * count when the frame was rendered by the canonical traversal (setting
 * empty_boxes = 0, trees without a coarse table, the array branch); with the
 * tree's empty boxes (the default where they exist) the reads THAT traversal
 * made: fewer, it skips nodes.  vrc_memory_usage2().empty_boxes says which.   */
int vrc_read_hits(vrc_caster *h, int32_t *hits, size_t n_int32);
#define VRC_HIT_FLAG_WRITTEN     1
#define VRC_HIT_FLAG_SHADOW_CAST 2
#define VRC_HIT_FLAG_SHADOW_HIT  4
#define VRC_HIT_FLAG_OOB_EXIT    8

/* ---- ray queries --------------------------------------------------------- */

/* What does a ray hit?  Picking (the voxel under the cursor), ground height (a ray straight down), collision and line of
 * sight, against the scene the handle renders -- also trees that exist only in device memory (vrc_build_shell_terrain,
 * vrc_build_heightfield), which have no host grid to cast against.
 *
 * A query is one ray, 6 floats: origin x, y, z, direction x, y, z.  It steps exactly like the primary ray of a frame whose
 * camera sits at the origin and whose ray is that direction (kernels/ray_caster_kernel.cl): the set-up of :298-323 without
 * the table rotation, then the loop of :557-570 -- step first, then test, so the origin voxel is never tested -- with the
 * frame's stop rule: materials 5 and 6 stop the ray, every other value passes through.  In the SVO branch a solid voxel's
 * material comes from the attachments when they are assigned, else it is 5.  The branch follows the settings as a frame
 * does: using_octree != 0 reads the dense map, 0 the tree.
 *
 * Two modes (flags):
 *   VRC_RAY_AS_PIXEL  the frame's own rules: the octree bias of :342-354 is computed for the origin's voxel exactly as a
 *                     frame computes it for a camera there (setting octree_bias honoured; in both branches, as in a frame),
 *                     and a direction with a zero component is rejected (:293-294).  Casting a frame's own pixel rays --
 *                     the viewport table rotated on the host with the frame's sin / cos (vrc_assign_camera_trig) -- gives
 *                     that frame's hit records: picking returns what the user sees.
 *   0 (default)       no bias, and zero components are allowed: an axis whose delta_t is +inf (a zero component, or one so
 *                     small that 1 / d overflows) gets delta_t = t = +inf and never steps.  Ground-height and axis-aligned
 *                     collision rays need this.
 * Both modes reject a ray with a non-finite component and a zero direction.
 *
 * max_steps caps distance_traveled like the setting max_distance caps a frame's; 0 means no cap below the map's edge (the
 * kernel bounds a ray at 3 * dim + 3 iterations, dim the largest map side).  Origins are expected in [0, dim)^3; a ray
 * that starts outside is stepped as a frame's would be -- the bounds test follows each step -- so it leaves on its first
 * iteration unless that step enters the map.
 *
 * out receives 8 x int32 per ray:
 *   [0..2] the voxel hit, or -1        [3] its material (5 / 6), or 0      [4] face bits of the entering step (bit0 x, bit1 y, bit2 z), or 0
 *   [5] VRC_RAY_* flags                [6] distance_traveled when the hit block would run (at the exit / the cap for a miss)
 *   [7] the float bits of min(intersection_t) at the entering iteration, before its increment: the entry parameter along the
 *       direction (biased under VRC_RAY_AS_PIXEL); for a miss the value at the last iteration; 0 for a rejected ray.
 * Fields 0-4 and 6 mean what fields 0-4 and 6 of vrc_read_hits mean for a frame rendered with shadow_rays = 0.
 *
 * Queries never change what a frame reports: counters, timing, hit records and the image stay those of the last frame.
 * Both calls are synchronous: they enqueue on the handle's stream (a frame in flight from vrc_compute_async finishes
 * first) and return when the records are written.  They use the coarse table and the empty boxes when vrc_prepare /
 * vrc_validate / a frame has built them (trees with box records for the upper levels only use them where they exist), and
 * otherwise run without them with the same results: a query never starts a derived build.  A group handle queries on
 * rank 0's GPU (the scene is replicated); the caller's current device is left as it was.  Errors, with nothing launched:
 * VRC_ERR_INVALID_ARGUMENT for a null handle / pointer, n < 0, max_steps < 0 or unknown flag bits; VRC_ERR_NOT_READY
 * before a successful vrc_validate or without a scene.  n = 0 succeeds.
 *
 * vrc_cast_rays: host arrays (float[6 * n] in, int32[8 * n] out), staged through device buffers that grow on demand and
 * are freed by vrc_release_map / _octree / _viewport and vrc_destroy.
 * vrc_cast_rays_device: device pointers on the handle's GPU (a torch tensor's data_ptr(), say), 4-byte aligned.  Work
 * queued on the null stream before the call is waited for; work on other streams is the caller's to finish first.      */
#define VRC_RAY_AS_PIXEL 1u
#define VRC_RAY_HIT       1
#define VRC_RAY_LEFT_MAP  2
#define VRC_RAY_STEP_CAP  4
#define VRC_RAY_REJECTED  8
int vrc_cast_rays(vrc_caster *h, const float *rays, int64_t n, int32_t max_steps, uint32_t flags, int32_t *out);
int vrc_cast_rays_device(vrc_caster *h, const void *d_rays, int64_t n, int32_t max_steps, uint32_t flags, void *d_out);

/* ---- box queries --------------------------------------------------------- */

/* Which voxels does a box overlap?  Map::BoxIntersection (include/map/Map.h:51, "the voxels that a box intersects /
 * contains"): the collision test of a player's or an object's AABB, the voxels an explosion or a brush touches, the terrain
 * inside a region -- against the scene the handle renders, device-built trees included.
 *
 * A box is 6 floats: origin x, y, z and extent x, y, z (the reference's origin and magnitude).  Per axis it covers the voxels
 * [lo, hi), lo = floor(o), hi = max(ceil(o + m), lo + 1), with o + m rounded to float32 first: the voxels [v, v + 1) that share
 * a point with the half-open box [o, o + m).  An axis with m = 0 is the plane at o, which lies in voxel floor(o); a box resting
 * on a face does not overlap the voxel below it.  The range is clipped to the map ([0, dim)^3 for the tree, map_dim for the
 * dense map); VRC_BOX_CLIPPED is set when any bound was clipped, and a box wholly outside gets count 0 and CLIPPED (it is not
 * rejected).  VRC_BOX_REJECTED: a non-finite component, a negative extent, or |o| or |o + m| >= 2^30; such a box is not
 * examined (count 0, corners -1, nothing listed).
 *
 * A voxel counts when its material is non-zero; with VRC_BOX_STOPPING_ONLY only when it is 5 or 6 (what stops a ray, the
 * rule of vrc_cast_rays).  The material is what a frame's hit test reads for the voxel, and the branch follows using_octree
 * as the ray queries do: the array branch reads the byte at the frame's index x + dx * (y + dz * z) (an index past the array
 * reads as empty); the SVO branch finds a voxel solid when it lies in a valid slot whose leaf bit is set, at any level, or in
 * any valid slot at the bottom level -- a valid leaf above the bottom is a solid cube of the slot's size, counted by volume --
 * with the attachment byte (int8) as the material for bottom-level descriptors when attachments are assigned, else 5.
 *
 * Per box i:
 *   records[8 i + 0]      VRC_BOX_* flags: ANY (count > 0), TRUNCATED (max_voxels > 0 and count > max_voxels), CLIPPED, REJECTED
 *   records[8 i + 1..3]   the per-axis minimum of the counted voxels; [4..6] the per-axis maximum (inclusive); -1 when
 *                         nothing counts (ground height under an AABB is [6], penetration extents without a list)
 *   records[8 i + 7]      entries written to the list: min(count, max_voxels); 0 for a rejected box
 *   counts[i]             the exact number of counted voxels (int64)
 *   voxels                may be null iff max_voxels == 0.  Box i owns entries [i max_voxels, (i + 1) max_voxels), each 4 int32
 *                         (x, y, z, material): the first min(count, max_voxels) counted voxels in Morton order (key bit 3k = x
 *                         bit k, 3k + 1 = y bit k, 3k + 2 = z bit k -- the tree's own child-slot order), so truncation is
 *                         deterministic and a full list is sorted.  Entries past records[8 i + 7] are not written.
 *
 * Everything else is as vrc_cast_rays: synchronous on the handle's stream (a frame in flight finishes first); the image, hit
 * records, counters and timing are untouched; the coarse table is used when vrc_prepare / vrc_validate / a frame has built it
 * and otherwise the query descends from the root with the same results (a query never starts a derived build); a group
 * handle queries on rank 0's GPU and the caller's current device is left as it was; the host call's staging and the scratch
 * of both calls grow on demand and are freed by vrc_release_map / _octree / _viewport and vrc_destroy.  Device pointers must be
 * memory the handle's GPU can read and write, 4-byte aligned, counts 8-byte aligned.  Errors, with nothing launched:
 * VRC_ERR_INVALID_ARGUMENT for a null handle or pointer, n < 0, max_voxels < 0, unknown flag bits or misalignment;
 * VRC_ERR_NOT_READY as for ray queries; VRC_ERR_LIMIT when n * max_voxels * 16 overflows size_t.  n = 0 succeeds.       */
#define VRC_BOX_STOPPING_ONLY 1u   /* flag: count only materials 5 and 6 (what stops a ray / vrc_cast_rays' rule) */
#define VRC_BOX_ANY        1       /* record[0] bits */
#define VRC_BOX_TRUNCATED  2
#define VRC_BOX_CLIPPED    4
#define VRC_BOX_REJECTED   8
int vrc_box_intersection(vrc_caster *h, const float *boxes, int64_t n, int32_t max_voxels, uint32_t flags,
                         int32_t *records, int64_t *counts, int32_t *voxels);
int vrc_box_intersection_device(vrc_caster *h, const void *d_boxes, int64_t n, int32_t max_voxels, uint32_t flags,
                                void *d_records, void *d_counts, void *d_voxels);

/* ---- swept-box queries --------------------------------------------------- */

/* How far can a box move before it touches something, and which face stops it?  Map::ShortRayIntersection
 * (include/map/Map.h:53, a stub in the reference) and the "collision result" its design note asks for: the move of a player,
 * a falling object or a projectile with volume, per tick -- with the contact normal that move-and-slide needs, and no
 * tunnelling through thin walls.
 *
 * A sweep is 9 floats: origin o, extent m (the box of vrc_box_intersection) and displacement d.  The box [o, o + m) moves to
 * [o + d, o + m + d) over t in [0, 1).  Which voxels count (VRC_SWEEP_STOPPING_ONLY = VRC_BOX_STOPPING_ONLY), which branch is
 * read, the materials, solid leaves above the bottom and out-of-map-is-empty are exactly vrc_box_intersection's rules above.
 *
 * The answer is defined by events, in float32 operations (unfused, IEEE divide, subnormals kept), so it can be replayed bit
 * for bit (tests/sweep_replay.py):
 *   start   per axis e = o + m rounded to float32, lo = floor(o), hi = max(ceil(e), lo + 1): the box query's range.  If that
 *           range, clipped to the map, holds a counted voxel: START_SOLID, t = 0, no normal, the voxel is the first counted
 *           voxel of the range in Morton order (the box query's list order), with its material.
 *   events  an axis moves iff d != 0.  With s = sign(d), its next leading event (the box enters a layer) is at
 *           t = ((float)hi - e) / d entering layer hi (s > 0), t = (o - (float)lo) / (-d) entering layer lo - 1 (s < 0); its
 *           next trailing event (the box leaves a layer) at t = ((float)(lo + 1) - o) / d leaving layer lo (s > 0),
 *           t = (e - (float)(hi - 1)) / (-d) leaving layer hi - 1 (s < 0) -- always from the current integer bound.  The event
 *           with the smallest t is next; ties: trailing before leading, then x < y < z.  No event, or not t < 1: the move is
 *           free, t = 1.  A trailing event shrinks the range by its layer.  A leading event tests the one-layer slab it enters
 *           (the current ranges of the other two axes, clipped to the map) and then extends the range; a counted voxel in the
 *           slab is a HIT: t = the event's time, normal code -s (a + 1) (+-1 x, +-2 y, +-3 z: the face normal of the blocking
 *           voxel, opposite to the motion), the voxel is the slab's first counted voxel in Morton order, with its material.
 *           A box resting on a face and moving into it hits at t = 0; moving along the face it does not touch the voxels below.
 *   stops   checked after the start test and after every event.  LEFT_MAP: on some axis hi <= 0 with d <= 0, or lo >= dim
 *           with d >= 0 (nothing can be met any more): free, t = 1.  EVENT_CAP: the next event has t < 1 but `cap` events
 *           were processed: t = the last processed event's time; cap = max_events, or 2 (dim_x + dim_y + dim_z) + 64 when
 *           max_events = 0.  CLIPPED: at the start or after some event a bound lay outside the map.
 *   REJECTED  what the box query rejects, a non-finite d, or |o + d| or |e + d| >= 2^30 (sums rounded to float32): flags only.
 *
 * Per sweep i, records[8 i + 0] VRC_SWEEP_* flags, [1] normal code (0: none), [2] the float bits of t, [3..5] the blocking
 * voxel (-1: none), [6] its material (0: none), [7] events processed (the event that hits included).  A rejected sweep has
 * t bits 0.
 *
 * Host rules as vrc_box_intersection: synchronous on the handle's stream, frame state and vrc_last_kernel untouched, the
 * coarse table used when it is built and never built here, rank 0's GPU for a group, the caller's device restored, staging
 * and scratch grown on demand and freed by vrc_release_map / _octree / _viewport and vrc_destroy, device pointers 4-byte
 * aligned.  Errors, with nothing launched: VRC_ERR_INVALID_ARGUMENT for a null handle or pointer, n < 0, max_events < 0,
 * unknown flag bits or misalignment; VRC_ERR_NOT_READY as for ray queries.  n = 0 succeeds.                              */
#define VRC_SWEEP_STOPPING_ONLY 1u     /* flag: only materials 5 and 6 block (vrc_cast_rays' rule); default: any non-zero material */
#define VRC_SWEEP_HIT          1       /* record[0] bits */
#define VRC_SWEEP_START_SOLID  2
#define VRC_SWEEP_CLIPPED      4
#define VRC_SWEEP_REJECTED     8
#define VRC_SWEEP_EVENT_CAP   16
#define VRC_SWEEP_LEFT_MAP    32
int vrc_sweep_boxes(vrc_caster *h, const float *sweeps, int64_t n, int32_t max_events, uint32_t flags, int32_t *records);
int vrc_sweep_boxes_device(vrc_caster *h, const void *d_sweeps, int64_t n, int32_t max_events, uint32_t flags, void *d_records);

/* ---- voxel reads ---------------------------------------------------------- */

/* What is in the scene?  Map::getVoxel (src/map/Map.cpp:25-29, a read of the reference's own host array) as a batch, and dense
 * blocks of materials -- for a mesher, a physics engine's chunk cache, a minimap, a save file -- against the scene the handle
 * renders, device-built trees included: those exist only on the GPU, so there is no host grid to look at.
 *
 * The material of voxel (x, y, z) is vrc_box_intersection's, and the branch follows using_octree: the array branch reads the
 * byte at the frame's index x + dx * (y + dz * z) (an index past the array reads as 0, a position outside map_dim reads as 0);
 * the SVO branch finds the voxel solid when it lies in a valid slot whose leaf bit is set, at any level, or in any valid slot
 * at the bottom level, with the attachment byte (int8, sign kept) as the material for bottom-level descriptors when
 * attachments are assigned, else 5; outside [0, dim)^3 is 0.  There is no STOPPING_ONLY filter: the caller gets the byte.
 *
 * vrc_get_voxels     positions int32[3 n], out int32[n]: out[i] = the material of voxel positions[3 i .. 3 i + 2], sign-extended.
 * vrc_read_regions   n regions of one common size (sx, sy, sz), each axis >= 1; lo int32[3 n], region i covers
 *                    [lo_i, lo_i + size) and owns bytes [i V, (i + 1) V) of out, V = sx sy sz:
 *                      out[i V + (x - lo.x) + sx * ((y - lo.y) + sy * (z - lo.z))] = the material of (x, y, z)
 *                    -- an int8[z][y][x] block, the layout vrc_build_dense_grid takes, so a scene can be read, changed on the
 *                    host and built again.  Every one of the n V bytes is written, zeros included; a region may lie partly or
 *                    wholly outside the map (that part is zeros: the one-voxel apron a mesher needs at the map's edge), and lo
 *                    may be any int32.  n_bytes is the size of out and must be at least n V.
 *
 * Host rules as vrc_box_intersection: synchronous on the handle's stream (a frame in flight finishes first); the image, hit
 * records, counters, timing and vrc_last_kernel are untouched; the coarse table is used when it is built and never built here,
 * with the same results without it; rank 0's GPU for a group, the caller's device restored; the host calls' staging grows on
 * demand and is freed by vrc_release_map / _octree / _viewport and vrc_destroy.  A read is one kernel launch with no scratch
 * and no host wait before the end.  The _device variants take memory the handle's GPU can read and write and wait for the
 * null stream first; positions, lo and the point output must be 4-byte aligned, the region output may have any alignment.
 * Errors, with nothing launched: VRC_ERR_INVALID_ARGUMENT for a null handle or pointer, n < 0, a size component < 1, a
 * misaligned 4-byte pointer or n_bytes < n V; VRC_ERR_LIMIT when n V overflows size_t (or exceeds 2^63);
 * VRC_ERR_NOT_READY as for ray queries.  n = 0 succeeds.                                                                  */
int vrc_get_voxels(vrc_caster *h, const int32_t *positions, int64_t n, int32_t *out);
int vrc_get_voxels_device(vrc_caster *h, const void *d_positions, int64_t n, void *d_out);
int vrc_read_regions(vrc_caster *h, const int32_t *lo, int64_t n, const int32_t size[3], int8_t *out, size_t n_bytes);
int vrc_read_regions_device(vrc_caster *h, const void *d_lo, int64_t n, const int32_t size[3], void *d_out, size_t n_bytes);

/* ---- exposed faces -------------------------------------------------------- */

/* Where is the scene's surface?  The exposed voxel faces of n regions -- for a mesher, a physics engine's collision geometry, a
 * minimap, a navigation builder, an instance buffer -- without moving the regions' voxels to the host: a terrain's surface is a
 * thin shell, and after vrc_set_voxels / vrc_fill_boxes only the touched chunks are extracted again.  Read-only.
 *
 * The material of voxel (x, y, z) is vrc_get_voxels', in either branch (the branch follows using_octree); outside the scene it
 * is 0.  A voxel is SOLID when its material is non-zero; with VRC_FACES_STOPPING_ONLY only when its material is 5 or 6 -- every
 * other value then counts as empty, as an owner and as a neighbour: the mesh of what the renderer draws.  Directions d = 0 .. 5
 * stand for -x, +x, -y, +y, -z, +z.  Face (v, d) exists when v is solid, v lies in its region and in the scene, and the
 * neighbour v + e_d is not solid.  The neighbour is read from the SCENE, not from the region: no face appears on a chunk seam
 * inside solid ground, and regions that tile the map yield disjoint face sets whose union is the whole map's set.  A neighbour
 * outside the scene is empty, so the map's own sides and bottom are faces; VRC_FACES_NO_MAP_EDGE drops exactly the faces whose
 * neighbour lies outside the scene.
 *
 * lo and size are vrc_read_regions': n regions [lo_i, lo_i + size) of one common size, lo int32[3 n], any int32; a region may
 * lie partly or wholly outside the scene, and that part owns no faces.  counts int64[n] receives the faces of every region,
 * always exact.  faces int32[4 capacity] receives the packed list: an entry is x, y, z, code with code = d | (material & 0xff)
 * << 8, and region i's entries start at the sum of counts[0 .. i).  Inside a region the faces are sorted by the brick coordinate
 * (v >> 3) - (lo_i >> 3), z-major (brick z, then brick y, then brick x), then by v.z, v.y, v.x, then by d.  Entries at or beyond
 * `capacity` are not written and memory past the written entries is not touched.  faces may be NULL iff capacity == 0: a
 * count-only call.  info may be NULL; set info->struct_size = sizeof(vrc_faces_info) before the call.
 *
 * Host rules as vrc_box_intersection: synchronous on the handle's stream (a frame in flight finishes first); the image, hit
 * records, counters, timing and vrc_last_kernel are untouched; the coarse table is used when it is built and never built here,
 * with the same results without it; rank 0's GPU for a group, the caller's device restored; staging and scratch grow on demand
 * and are freed by vrc_release_map / _octree / _viewport and vrc_destroy.  One host wait in the middle: the total sizes the
 * list pass, which runs only when capacity > 0.  The _device variant takes memory the handle's GPU can read and write and waits
 * for the null stream first; d_lo and d_faces must be 4-byte aligned, d_counts 8-byte aligned.
 * Errors, with nothing launched: VRC_ERR_INVALID_ARGUMENT for a null handle or a null required pointer, n < 0, a size
 * component < 1, capacity < 0, unknown flag bits, misalignment or an info whose struct_size is below 4; VRC_ERR_LIMIT when
 * n times the bricks a region can touch ((size + 6) / 8 + 1 per axis) exceeds 2^31 - 1 or capacity * 16 overflows size_t;
 * VRC_ERR_NOT_READY as for ray queries.  n = 0 succeeds.                                                                      */
#define VRC_FACES_NO_MAP_EDGE   1u
#define VRC_FACES_STOPPING_ONLY 2u
typedef struct vrc_faces_info {         /* size-versioned like vrc_edit_info */
    uint32_t struct_size;               /* in: sizeof the caller's struct; out: bytes written */
    uint32_t truncated;                 /* 1 when faces_total > capacity */
    int64_t  faces_total;               /* the sum of counts */
    int64_t  faces_written;             /* min(faces_total, capacity) */
    double   seconds;                   /* device time of the call's kernels */
} vrc_faces_info;
int vrc_extract_faces(vrc_caster *h, const int32_t *lo, int64_t n, const int32_t size[3], int64_t capacity, uint32_t flags,
                      int64_t *counts, int32_t *faces, vrc_faces_info *info);
int vrc_extract_faces_device(vrc_caster *h, const void *d_lo, int64_t n, const int32_t size[3], int64_t capacity, uint32_t flags,
                             void *d_counts, void *d_faces, vrc_faces_info *info);

/* ---- voxel edits ---------------------------------------------------------- */

/* Change the scene.  Map::setVoxel / ArrayMap::setVoxel (include/map/Map.h:42, ArrayMap.h:17) as a batch against the scene the
 * handle renders: dig a hole, place a block, without reading the scene back and building it again -- which is a PCIe round trip
 * of the whole grid, ends at depth 12 and does not exist for the trees that live only in HBM (vrc_build_shell_terrain,
 * vrc_build_heightfield).
 *
 * positions int32[3 n], materials int32[n], each in [-128, 127]: the int8 vrc_get_voxels sign-extends; 0 clears the voxel.
 * After the call vrc_get_voxels / vrc_read_regions return what applying the edits IN INDEX ORDER to the scene before the call
 * gives: the highest index wins a position that occurs more than once.  An edit outside the scene -- [0, dim)^3 for the tree;
 * map_dim, or an index past the array, for the map -- is ignored and counted in `skipped`.  Which scene is edited follows
 * using_octree, as for the queries; a host that keeps both scenes makes two calls.  flags must be 0.  info may be NULL; set
 * info->struct_size = sizeof(vrc_edit_info) before the call (never more than that is written).
 *
 * Array branch: a scatter into the map at the frame's index x + dx * (y + dz * z).
 *
 * SVO branch: a path-copying, APPEND-ONLY edit.  Every touched brick (a map-aligned cube of min(8, dim) voxels) is read, changed
 * and rebuilt by one wave, every touched node above the bricks gets a new child block whose untouched children point, by far
 * pointers, into the old array, and a new root word is appended; the last step moves n_descriptors and the octree_root_index
 * setting of the handle (and of every rank of its group).  The edited tree is the tree vrc_build_dense_grid(...,
 * VRC_BUILD_ATTACHMENTS) builds from the edited grid, up to layout: the same node at every position, the same (valid, leaf)
 * masks, empty subtrees pruned up to the root (an empty scene is a root with valid mask 0), solid regions never collapsed into
 * leaves; a solid leaf above the bottom level that is dug into becomes an ordinary node whose untouched children are leaves.
 * Images, hit records and canonical read counts equal those of the rebuilt tree.
 *   - Placement is a function of (array before the call, batch) alone: two handles with equal arrays that receive the same batch
 *     end with bit-identical arrays.
 *   - Growth: descriptors_added <= 72 * bricks_touched + 16 * (touched nodes above the bricks) + 1; words of the appended range
 *     that hold nothing are zero.  Old words are never overwritten, so every edit leaves garbage behind and the array grows
 *     with every batch; vrc_compact_octree (below) drops the garbage and puts the tree back into a dense layout, at any depth
 *     and for trees that live only in HBM.
 *   - A batch that changes no voxel (voxels_changed == 0) appends nothing and leaves the root where it was.
 *   - Materials: every rebuilt bottom-level descriptor gets an attachment slot of its own.  A tree without attachments stays
 *     without them while every written material is 0 or 5 (trees that live only in HBM must not suddenly need 4 bytes per
 *     descriptor); the first other material creates the lookup (all zeros) and slot 0 = eight 5s, and failing to allocate them is
 *     VRC_ERR_OUT_OF_MEMORY with nothing changed.
 *   - Capacity: when the batch does not fit what is allocated, the arrays are allocated anew with `edit_reserve` words to spare
 *     and copied device to device (old and new exist side by side for that moment).  Setting edit_reserve: -1 (default) = an
 *     eighth of the new size, at least 4096 words and at most a sixteenth of the free device memory; 0 = exact; n = n words.
 *     vrc_octree_size and vrc_read_descriptors report n_descriptors; vrc_memory_usage*'s octree_bytes reports what is allocated.
 *   - The coarse table and the empty boxes describe the old tree and are dropped; vrc_prepare, vrc_validate or the next
 *     vrc_compute that finds them missing builds them again (about 15 ms for the table, 0.6 s for the boxes at depth 12).
 *     Queries never start such a build and give the same results without them.  A host that edits every frame sets
 *     empty_boxes = 0.
 *   - A group handle replicates the call: ranks that share rank 0's tree only take the new root, ranks with their own copy run
 *     the same edit on their GPU.  A tree that is also held by a handle OUTSIDE the caller's group (vrc_assign_octree_from)
 *     is refused with VRC_ERR_LIMIT and nothing changes: that holder's octree_root_index cannot be moved from here.
 *
 * Host rules as vrc_box_intersection: synchronous on the handle's stream (a frame in flight finishes first); the image, hit
 * records, counters, timing and vrc_last_kernel are untouched; the caller's device is restored; staging and scratch grow on
 * demand and are freed by vrc_release_map / _octree / _viewport and vrc_destroy.  The _device variant takes memory the handle's
 * GPU can read, 4-byte aligned, and waits for the null stream first; it cannot check the materials without a read-back, so an
 * out-of-range material there makes that edit `skipped`.
 * Errors, with nothing launched and nothing changed: VRC_ERR_INVALID_ARGUMENT for a null handle or pointer, n < 0, flags != 0,
 * a misaligned device pointer, an info whose struct_size is below 4 or (host call) a material outside [-128, 127]; VRC_ERR_LIMIT for n > 2^31 - 1; VRC_ERR_NOT_READY
 * as for ray queries.  n = 0 succeeds and changes nothing.  The edit is atomic: on any failure, VRC_ERR_OUT_OF_MEMORY while
 * growing the arrays included, the scene, n_descriptors and the root are what they were.                                      */
typedef struct vrc_edit_info {          /* size-versioned like vrc_memory2 */
    uint32_t struct_size;               /* in: sizeof the caller's struct; out: bytes written */
    uint32_t reserved_;
    int64_t  skipped;                   /* edits outside the scene (ignored) */
    int64_t  voxels_changed;            /* voxels whose material differs after the batch */
    int64_t  bricks_touched;            /* SVO branch: map-aligned bricks rewritten; array branch: 0 */
    uint64_t descriptors_added;         /* words the array grew by (descriptors, far slots and filler) */
    uint64_t n_descriptors, root_index; /* the tree after the edit (SVO branch) */
    double   seconds;                   /* device time of the edit's kernels */
} vrc_edit_info;
int vrc_set_voxels(vrc_caster *h, const int32_t *positions, const int32_t *materials, int64_t n, uint32_t flags, vrc_edit_info *info);
int vrc_set_voxels_device(vrc_caster *h, const void *d_positions, const void *d_materials, int64_t n, uint32_t flags, vrc_edit_info *info);

/* ---- region edits --------------------------------------------------------- */

/* Change whole regions of the scene: fill axis-aligned boxes with a material (dig a crater, carve a corridor, paint a wall) and
 * paste dense int8 blocks (stamp a prefab) -- the inverse of vrc_read_regions -- without expanding the shape into one
 * (x, y, z, material) tuple per voxel.  An operation is six integers; no voxel of it is enumerated on the host or on the device.
 *
 * Operations
 *   vrc_fill_boxes      boxes int32[6 n]: lo x, y, z, then size x, y, z, every size >= 1; box i covers [lo, lo + size).
 *                       materials int32[n], each in [-128, 127]; 0 clears.
 *   vrc_write_regions   exactly the arguments and the block layout of vrc_read_regions: n regions of one common size
 *                       (sx, sy, sz), lo int32[3 n], region i owns bytes [i V, (i + 1) V) of data, V = sx sy sz, and byte
 *                       (x - lo.x) + sx * ((y - lo.y) + sy * (z - lo.z)) of region i is the material for (x, y, z).
 *                       n_bytes is the size of data and must be at least n V.
 *   lo may be any int32; lo + size is formed in 64 bits: a box at lo = INT32_MIN with size INT32_MAX is legal.  The part of an
 *   operation outside the scene -- [0, dim)^3 for the tree; map_dim, or an index past the array, for the map -- is ignored
 *   without comment.  An operation that touches no voxel of the scene is counted in info->skipped.  In the _device fill variant
 *   an operation with a material outside [-128, 127] or a size < 1 cannot be refused without a read-back: it is skipped and
 *   counted; the host call refuses it with VRC_ERR_INVALID_ARGUMENT.
 *
 * Order.  The result is what applying the operations IN INDEX ORDER gives: operation i sees the scene as operations 0 .. i-1
 * left it.  That decides overlaps, and it decides the flags, which test the material a voxel has at that moment:               */
#define VRC_WRITE_WHERE_EMPTY 1u   /* write only voxels whose material is 0 at that moment (build, never overwrite) */
#define VRC_WRITE_WHERE_SOLID 2u   /* write only voxels whose material is non-zero at that moment (paint, dig) */
#define VRC_WRITE_SKIP_ZERO   4u   /* vrc_write_regions only: a 0 byte of the block leaves the voxel alone (stamp a prefab) */
/* WHERE_EMPTY | WHERE_SOLID together is VRC_ERR_INVALID_ARGUMENT; so is SKIP_ZERO on a fill, and so is any other bit.
 *
 * Everything else is vrc_set_voxels' contract.  The branch follows using_octree.  The SVO edit is the same append-only,
 * path-copying edit with the same commit: the edited tree is the tree vrc_build_dense_grid(..., VRC_BUILD_ATTACHMENTS) builds
 * from the edited grid, up to layout, empty subtrees pruned up to the root, solid regions never collapsed into leaves; the same
 * growth bound (descriptors_added <= 72 * bricks_touched + 16 * touched nodes above the bricks + 1), the same edit_reserve,
 * the same atomicity on every failure, the coarse table and the empty boxes dropped the same way; a group replicates the call
 * the same way and a tree held outside the group is VRC_ERR_LIMIT.  The host rules and vrc_edit_info are the same, where
 * `skipped` counts operations and `bricks_touched` counts every brick that the in-scene part of an operation overlaps, whether
 * or not the brick changed (array branch: 0).  A batch that changes no voxel appends nothing, leaves the root where it was and
 * reports bricks_touched = descriptors_added = 0, as vrc_set_voxels does.
 *
 * Placement is a function of (array before the call, set of touched bricks, resulting voxels) alone: the touched bricks sit in
 * Morton-key order at brick_base + 72 u and the ancestors are appended exactly as vrc_set_voxels appends them.  So with
 * flags = 0 a fill produces an array, a lookup and attachments bit-identical to those vrc_set_voxels produces for the same
 * boxes expanded to their in-scene positions in operation order, and so does a paste.
 *
 * Materials.  A tree without attachments stays without them when every fill operation that touches the scene has material 0
 * or 5 and every byte of the in-scene part of every pasted region is 0 or 5 -- whatever the flags are, so the decision is a
 * function of the batch and the scene size alone.  Otherwise the lookup and slot 0 are created as vrc_set_voxels creates them.
 *
 * Array branch.  Fills and pastes go into the map at the frame's index x + dx * (y + dz * z).  A map with dy > dz, where that
 * index is not one-to-one over map_dim, is refused with VRC_ERR_LIMIT and nothing is changed.
 *
 * Limits.  VRC_ERR_LIMIT when n > 2^31 - 1, when the batch has more than 2^31 - 1 (brick, operation) pairs -- a pair is one
 * map-aligned 8^3 brick overlapped by one operation -- or when n V overflows size_t (or exceeds 2^63), as in vrc_read_regions.
 * VRC_ERR_OUT_OF_MEMORY, with nothing changed, when the appended range does not fit: a fill of a whole deep map is such a case.
 * The _device variants take memory the handle's GPU can read and wait for the null stream first; boxes, materials and lo must
 * be 4-byte aligned, the blocks may have any alignment.
 * Errors, with nothing launched and nothing changed: VRC_ERR_INVALID_ARGUMENT for a null handle or pointer, n < 0, the flag
 * combinations above, a size component < 1 (host fill and both pastes), n_bytes < n V, a misaligned device pointer, an info
 * whose struct_size is below 4 or (host fill) a material outside [-128, 127]; VRC_ERR_NOT_READY as for ray queries.  n = 0
 * succeeds and changes nothing.                                                                                              */
int vrc_fill_boxes(vrc_caster *h, const int32_t *boxes, const int32_t *materials, int64_t n, uint32_t flags, vrc_edit_info *info);
int vrc_fill_boxes_device(vrc_caster *h, const void *d_boxes, const void *d_materials, int64_t n, uint32_t flags, vrc_edit_info *info);
int vrc_write_regions(vrc_caster *h, const int32_t *lo, int64_t n, const int32_t size[3], const int8_t *data, size_t n_bytes, uint32_t flags, vrc_edit_info *info);
int vrc_write_regions_device(vrc_caster *h, const void *d_lo, int64_t n, const int32_t size[3], const void *d_data, size_t n_bytes, uint32_t flags, vrc_edit_info *info);

/* ---- shape fills ---------------------------------------------------------- */

/* Fill balls and axis-aligned cylinders with a material: an explosion crater, a round tunnel, a well, a pillar.  vrc_fill_boxes
 * with round operations: an operation is still six integers, and no voxel of it is enumerated on the host or on the device.
 *
 * shapes int32[6 n]: kind, cx, cy, cz, r, h.  materials int32[n], each in [-128, 127]; 0 clears.                              */
#define VRC_SHAPE_BALL        0
#define VRC_SHAPE_CYLINDER_X  1
#define VRC_SHAPE_CYLINDER_Y  2
#define VRC_SHAPE_CYLINDER_Z  3
/* Membership is defined in integers, so a host can replay it exactly:
 *   ball                       voxel v is in the shape iff (vx - cx)^2 + (vy - cy)^2 + (vz - cz)^2 <= r^2; r = 0 is the single
 *                              voxel c; h must be 0.
 *   cylinder along a = kind-1  voxel v is in the shape iff c_a <= v_a < c_a + h and the squared distance over the other two
 *                              axes is <= r^2; h >= 1; c_a + h is formed in 64 bits (c_a = INT32_MAX - 1 with h = INT32_MAX is
 *                              legal).
 *   0 <= r <= 2^30; c may be any int32.  An axis with |d| > r is outside and is tested first; after that every square is at most
 *   2^60 and every sum fits signed 64 bits, so nothing wraps and nothing rounds (the one square root, the half width of a row, is
 *   an exact integer root).
 * An operation is invalid when its kind is unknown, r is outside [0, 2^30], a ball has h != 0, a cylinder has h < 1 or its
 * material is outside [-128, 127]: the host call refuses the batch with VRC_ERR_INVALID_ARGUMENT and changes nothing; the _device
 * call, which cannot look without a read-back, skips that operation and counts it in info->skipped.
 *
 * Everything else is vrc_fill_boxes' contract, with "shape" for "box": the operations apply IN INDEX ORDER; flags are
 * VRC_WRITE_WHERE_EMPTY or VRC_WRITE_WHERE_SOLID, which exclude each other (VRC_WRITE_SKIP_ZERO and any other bit:
 * VRC_ERR_INVALID_ARGUMENT); the branch follows using_octree; the part of a shape outside the scene is ignored and an operation
 * with no voxel in the scene is counted in `skipped`; a tree without attachments stays without them while every operation that
 * has a voxel in the scene has material 0 or 5; the growth bound, edit_reserve, atomicity, the dropped coarse table and boxes, the
 * group's replication, VRC_ERR_LIMIT for a tree held outside the group, for a map with dy > dz, for n > 2^31 - 1 and for more
 * than 2^31 - 1 (brick, operation) pairs, the _device variant's pointers and the host rules are the fills'.
 *
 * What differs: `bricks_touched`.  A brick is touched iff it holds at least one in-scene voxel of some valid operation -- the
 * exact set, not the bricks of the bounding box -- and a pair is one such brick of one operation.  That keeps the placement
 * promise: with flags = 0 the descriptor array, the lookup and the attachments are bit-identical to those vrc_set_voxels
 * produces for the shapes expanded to their in-scene voxels in operation order.  A batch that changes no voxel appends nothing.
 * Cost: the front end takes one step per brick row (by, bz) of each shape's bounding box clipped to the scene, the brick pass
 * one wave per touched brick; nothing scales with r^3.                                                                          */
int vrc_fill_shapes(vrc_caster *h, const int32_t *shapes, const int32_t *materials, int64_t n, uint32_t flags, vrc_edit_info *info);
int vrc_fill_shapes_device(vrc_caster *h, const void *d_shapes, const void *d_materials, int64_t n, uint32_t flags, vrc_edit_info *info);

/* ---- octree compaction ---------------------------------------------------- */

/* Copy the part of the descriptor array that the root reaches into a new, dense, canonically ordered array on the device, remap
 * the materials, and install the result as an edit's commit does: what vrc_set_voxels leaves behind -- the orphaned paths, the
 * 72-word brick stride, the far pointers into the old array -- is gone, n_descriptors shrinks to the live tree and the root moves
 * to index 0.  The scene does not change: reads, queries, frames, hit records and canonical counters are those of before.
 *
 * The new array.  n = log2(dim); a descriptor at level l (root: 0) is BOTTOM-LEVEL when l = n - 1 and HOLDS A POINTER when
 * l < n - 1 and its valid mask is non-zero.  reach = setting compact_near_reach (default 0x7fff, range [16, 0x7fff]).  For a
 * descriptor D that holds a pointer, with kept children c_0 .. c_{m-1} in slot order: P(c_k) = 1 when c_k's slot is no leaf slot
 * and c_k holds a pointer; the subtree words S(c) are 0 when P(c) = 0; c_k is FAR when P(c_k) and 16 + sum_{j<k} S(c_j) > reach;
 * f = the number of far children; S(D) = m + f + sum_k S(c_k).  Placement is pre-order: the root at index 0, its child block at
 * 1; a child block at B holds the children at B .. B+m-1, the far slots of the far children (in child order) at B+m .. B+m+f-1,
 * then the children's own blocks in child order, c_k's at T_k = B + m + f + sum_{j<k} S(c_j).  A near pointer is T_k - (B+k); a
 * far pointer is 0x8000 | (slot - (B+k)) and the slot holds T_k.  (The far rule is pessimistic on purpose: the constant 16 --
 * eight words and eight far slots -- makes it computable bottom-up.)  Every copied word keeps bits 16-63 of the old word; bits
 * 0-15 are the new pointer, zero where no walker follows one (bottom-level descriptors, valid mask 0, the words of leaf slots).
 * n_descriptors = 1 + S(root), and every word is the root, a word of a reachable child block or a far slot one descriptor names.
 * The layout is a function of the tree alone: two arrays that encode the same tree (with the same words in their leaf slots)
 * compact to identical arrays, and compacting twice in a row leaves the array bit-identical.
 *
 * Materials.  A tree without attachments stays without.  Otherwise the attachment slots named by the lookup of a reachable
 * bottom-level descriptor are kept, in increasing old-slot order, and the rest are dropped; descriptors that shared a slot still
 * share it; lookup[new] is the remapped slot for a bottom-level descriptor and 0 for every other word.  (When no descriptor names
 * a slot, one slot of eight 5s stays: a tree with materials never has an empty attachment array.)
 *
 * Host.  Out of place: the new arrays are allocated at their size + edit_reserve (the edit's rule) BESIDE the old ones, which are
 * freed at the commit once the device is idle; a tree that does not fit twice is VRC_ERR_OUT_OF_MEMORY (in-place compaction does
 * not exist).  Atomic: on any failure nothing has changed.  The commit moves n_descriptors, octree_root_index (to 0),
 * n_attachments and the capacities, and drops the coarse table and the empty boxes as an edit does.  A group handle replicates
 * the call: ranks that share rank 0's tree take the new root, ranks with their own copy run the same compaction (the layout is
 * canonical, so the copies stay equal); a tree also held OUTSIDE the group is VRC_ERR_LIMIT, as for edits.  Otherwise the host
 * rules of vrc_set_voxels: synchronous on the handle's stream; image, records, counters, timing and vrc_last_kernel untouched;
 * the caller's device restored.  The call's scratch (about 42 bytes per pointer-holding descriptor, a fifth of a tree) is freed
 * before it returns.  using_octree != 0 (the array branch) succeeds and changes nothing.
 * flags: VRC_COMPACT_DRY_RUN measures only (the sizes, the far children, the used attachment slots), fills info and changes
 * nothing -- for a host that compacts when descriptors_before is a multiple of n_descriptors.  Any other bit, a null handle, an
 * info whose struct_size is below 4 or compact_near_reach outside its range: VRC_ERR_INVALID_ARGUMENT; VRC_ERR_NOT_READY as for
 * ray queries; an array whose pointers leave it or that is no tree: VRC_ERR_INVALID_ARGUMENT.                                 */
#define VRC_COMPACT_DRY_RUN 1u
typedef struct vrc_compact_info {       /* size-versioned like vrc_edit_info */
    uint32_t struct_size;               /* in: sizeof the caller's struct; out: bytes written */
    uint32_t reserved_;
    uint64_t descriptors_before;        /* n_descriptors before the call */
    uint64_t n_descriptors, root_index; /* the tree after the call (a dry run: as it would be) */
    uint64_t live_descriptors;          /* reachable words without far slots */
    uint64_t far_slots;
    uint64_t attachments_before, n_attachments;
    double   seconds;                   /* device time of the call's kernels */
} vrc_compact_info;
int vrc_compact_octree(vrc_caster *h, uint32_t flags, vrc_compact_info *info);

/* Device pointers of the resident frame buffers (float4[w*h], int32[8*w*h]);
 * lets a host that owns the GPU (e.g. a torch process) consume the frame
 * without a PCIe round trip.                                                 */
int vrc_device_image(vrc_caster *h, void **dev_ptr, size_t *n_bytes);

/* Counters of the most recent frame (device-side, fetched at sync). */
typedef struct vrc_counters {
    uint64_t primary_rays;
    uint64_t shadow_rays;
    uint64_t descriptor_reads;   /* SURVEY 8(d)'s canonical count, or the box traversal's own (see vrc_read_hits) */
    uint64_t texel_reads;
    uint64_t map_reads;
    uint64_t steps;
    uint64_t unwritten_pixels;
    uint64_t watchdog_trips;     /* wavefronts the kernel's round watchdog had to stop.  Always 0; anything else is a
                                    kernel bug: vrc_get_counters then returns VRC_ERR_DEVICE, the frame is invalid */
} vrc_counters;
int vrc_get_counters(vrc_caster *h, vrc_counters *out);
/* Which count descriptor_reads (and field 7 of the hit records) of the most recent frame is: *canonical = 1 when it is SURVEY
 * 8(d)'s canonical count -- the array branch, trees without a coarse table, setting empty_boxes = 0 -- and 0 when the frame was
 * rendered with the tree's empty boxes and the fields hold that traversal's own, smaller count.  So that one frame's records
 * describe themselves (a host that compares them with the oracle or the reference reads this instead of guessing from settings). */
int vrc_counters_canonical(vrc_caster *h, int32_t *canonical);
/* Which kernel rendered the most recent frame of one rank (rank 0 = the handle itself, as in vrc_memory_usage2): the launch
 * records the template arguments it instantiates the kernel with, so this is what ran, not a second derivation from the
 * settings.  Size-versioned like vrc_memory2: set struct_size = sizeof(vrc_kernel_info) before the call.
 * VRC_ERR_INVALID_ARGUMENT for a null handle / pointer or a rank outside the group, VRC_ERR_NOT_READY before the first frame.
 * A rank that owns no rows of the frame launched nothing: family VRC_KERNEL_NONE, empty name.                              */
#define VRC_KERNEL_NONE  0
#define VRC_KERNEL_SVO   1         /* raycast_svo_kernel<kJump, kMulti, kTuned, kLdsRows, kCoarse, kBox>: the exact mode */
#define VRC_KERNEL_JUMP  2         /* raycast_jump_kernel<kMulti, kCoarse>: stepping_mode 1 */
#define VRC_KERNEL_ARRAY 3         /* raycast_array_kernel: the dense map, no template arguments */
typedef struct vrc_kernel_info {
    uint32_t struct_size;             /* in: sizeof the caller's struct; out: bytes written */
    int32_t  family;                  /* VRC_KERNEL_* */
    int32_t  n_args;                  /* template arguments of the instance: 6, 2 or 0 */
    int32_t  args[6];                 /* their values in declaration order (bools as 0 / 1), -1 past n_args */
    int32_t  jump_min_run;            /* the frame's resolved threshold of the closed-form jumps; 1 << 24: it ran without them */
    int32_t  lds_rows;                /* rows of the jumps' Euclid tables in LDS: 3, 2, or 0 (global memory / no jumps) */
    int32_t  reserved_;
    char     name[96];                /* e.g. "raycast_svo_kernel<true, false, true, 3, true, true>" */
} vrc_kernel_info;
int vrc_last_kernel(vrc_caster *h, int32_t rank, vrc_kernel_info *out);

/* The index audit (csrc/index_audit.hpp; the audit build of the library, compiled with -DVRC_INDEX_AUDIT): every index the frame
 * kernels form into one of VRC_AUDIT_ARRAYS arrays is compared on the device with the extent the host layer allocated, counted,
 * and clamped where it is out of range.  Both calls exist in every build; in the product build they return VRC_ERR_NOT_READY
 * and touch nothing.  The audit build serialises its launches and serves one host thread.
 * vrc_index_audit_report: the counts since the last clear on GPU `device` (-1: the current one), summed over the library's
 * kernel files, for array ids 0 .. n_entries-1 (the order of index_audit.hpp's table); clear != 0 zeroes them.  extent is the
 * largest one published since the last clear to a kernel file that accessed the array (every access was checked against the one in
 * force when it was made; extent_published = 0: none, accesses are counted and not checked); max_index means
 * something when accesses > 0, the first_* fields when violations > 0 (first_site: the source line of the access).
 * vrc_index_audit_shrink (tests only): from now on publish array_id's extent smaller by `amount` elements (0: as allocated).  */
#define VRC_AUDIT_ARRAYS 24
typedef struct vrc_index_audit_entry {
    uint64_t accesses, max_index, extent, violations;
    int64_t  first_index;
    uint64_t first_extent;
    uint32_t first_block, first_site, extent_published, reserved_;
} vrc_index_audit_entry;
int vrc_index_audit_report(int32_t device, vrc_index_audit_entry *out, int32_t n_entries, int32_t clear);
int vrc_index_audit_shrink(int32_t array_id, uint64_t amount);

/* Wave-scheduler statistics of the SVO kernel for the most recent frame (per wave, not per lane):
 * [0] step-loop iterations, [1] bursts, [2] node-event passes, [3] lanes serviced in them,
 * [4] hit-block passes, [5] lanes shaded in them, [6..7] reserved.                */
int vrc_get_scheduler_stats(vrc_caster *h, uint64_t out[8]);

/* hipEvent timing of the raycast kernel on the handle's stream, accumulated
 * since the last reset (replaces GraphTimer "Compute", Application.cpp:151-155). */
int vrc_timing_reset(vrc_caster *h);
int vrc_timing_get(vrc_caster *h, uint64_t *n_launches, double *total_kernel_ms);

/* ---- SVO construction (host side) -------------------------------------- */

/* Octree::Generate (src/map/Octree.cpp:13-43,171-323): bottom-up build of the
 * descriptor array from a dense char[dim^3] grid.  buffer_size == 0 sizes the
 * array exactly; otherwise the array has buffer_size entries filled from the
 * end like the reference's fixed 100000-entry buffer (Octree.h:29).
 * strict_reference != 0 reproduces the reference layout bit for bit including
 * its far-pointer corner cases; 0 emits the same format with those fixed.
 * The result is malloc'ed; release with vrc_free.                            */
int vrc_octree_generate(const int8_t *grid, uint32_t dim, uint64_t buffer_size,
                        int strict_reference, uint64_t **descriptors,
                        uint64_t *n_descriptors, uint64_t *root_index);

/* Material attachments (layout: see vrc_assign_octree_attachments) for an array built from `grid`.
 * Results are malloc'ed; release with vrc_free.                                  */
int vrc_octree_attachments_from_grid(const int8_t *grid, uint32_t dim, const uint64_t *descriptors,
                                     uint64_t n_descriptors, uint64_t root_index, uint32_t **lookup,
                                     uint64_t **attachments, uint64_t *n_attachments);
/* ... and for the procedural scene: material 6 (mirror) where hash(x,y,z,seed) % mirror_period == 0,
 * else 5; mirror_period 0 = all 5.                                               */
int vrc_scene_shell_terrain_attachments(uint32_t depth, uint64_t seed, uint32_t mirror_period,
                                        const uint64_t *descriptors, uint64_t n_descriptors,
                                        uint64_t root_index, uint32_t **lookup, uint64_t **attachments,
                                        uint64_t *n_attachments);

/* Procedural sparse builder for grids too large to materialise (SURVEY 8d
 * "shell-terrain"): solid iff h(x,y)-thickness <= z <= h(x,y).  Emits the same
 * format/layout as vrc_octree_generate on the equivalent dense grid.
 * height: optional out, int32[dim*dim] (x + dim*y).                          */
int vrc_scene_shell_terrain(uint32_t depth, uint64_t seed, int32_t thickness,
                            int strict_reference, uint64_t **descriptors,
                            uint64_t *n_descriptors, uint64_t *root_index,
                            int32_t *height);
/* Dense twin of the above for depth <= 9 (fills char[dim^3] with material 5). */
int vrc_scene_shell_terrain_dense(uint32_t depth, uint64_t seed, int32_t thickness, int8_t *grid);
/* Map::GenerateHeightBitmap (src/map/Map.cpp:144-262): the reference's diamond-square height field
 * (std::mt19937 default seed, offsets in +-h with h = 20 halved per level, wrap-around sampling :266-272), whose
 * output the reference drops in the empty Map::ApplyHeightmap (:140-142).  height: uint8[dim*dim] =
 * clamp(value, 0, dim) like :241; corner_seed is the reference's `rand() % 10 + 55` (:160; 58 with an unseeded glibc).
 * grid (optional, int8[dim^3], x + dim*(y + dim*z)): what ApplyHeightmap was meant to do -- material 5 at and
 * below the height of each column, 0 above (our definition; the reference has none).  dim <= 4096 with a grid,
 * <= 16384 without (then feed the heights to vrc_build_heightfield: no dense grid anywhere).                    */
int vrc_scene_diamond_square(uint32_t dim, double corner_seed, uint8_t *height, int8_t *grid);
/* The same field before Map.cpp:248 quantises it: double[dim*dim], x + dim*y (what `height_map` holds at :244).  For
 * checks against a second implementation (oracle/diamond_square.py): the uint8 heights hide everything below one voxel. */
int vrc_scene_diamond_square_f64(uint32_t dim, double corner_seed, double *field);

/* The same scene with its knobs exposed: octave_floor = log2 of the finest noise cell (2 in vrc_scene_shell_terrain),
 * layout = VRC_LAYOUT_* flags.  VRC_LAYOUT_NO_PAGE_HEADERS is the "brick" layout the device builder emits: same
 * descriptor format and bottom-up order, no all-ones page-header slots (they are the only position-dependent part of
 * the reference layout, Octree.cpp:251-262, and neither kernel reads them).                                          */
#define VRC_LAYOUT_STRICT_REFERENCE 1u
#define VRC_LAYOUT_NO_PAGE_HEADERS  2u
int vrc_scene_shell_terrain_ex(uint32_t depth, uint64_t seed, int32_t thickness, int32_t octave_floor, uint32_t layout,
                               uint64_t **descriptors, uint64_t *n_descriptors, uint64_t *root_index, int32_t *height);
/* One column of that scene, evaluated procedurally: solid for lo <= z <= hi. */
int vrc_scene_shell_column(uint32_t depth, uint64_t seed, int32_t thickness, int32_t octave_floor, int64_t x, int64_t y,
                           int32_t *lo, int32_t *hi);

/* Builds the scene's SVO directly in the handle's HBM and installs it as the octree (no host copy ever exists):
 * replaces the reference builder's limits -- Octree::buffer_size = 100000 descriptors (include/map/Octree.h:29) and the
 * dense char[D^3] input of Octree::Generate (src/map/Octree.cpp:13,325-327).  The array is bit-identical to
 * vrc_scene_shell_terrain_ex(..., VRC_LAYOUT_NO_PAGE_HEADERS).  flags: VRC_BUILD_COUNT_ONLY sizes the tree without
 * allocating it.  validate_samples > 0 runs the reference's Octree::Validate (Octree.cpp:329-352) on the device over
 * that many pseudo-random voxels (tree point query vs the procedural occupancy).  probe_xy (n_probe x,y pairs) /
 * probe_lohi (n_probe lo,hi pairs): optional read-back of columns of the device height field.                      */
#define VRC_BUILD_COUNT_ONLY 1u
#define VRC_BUILD_ATTACHMENTS 2u   /* vrc_build_dense_grid: the grid's values become the tree's material attachments, on the device */
typedef struct vrc_build_info {
    uint64_t n_descriptors, root_index;
    uint64_t n_bricks, n_top_slots, n_far_pointers_top;
    double   seconds_total, seconds_height, seconds_count, seconds_emit;
    uint64_t device_bytes_peak;      /* descriptor array + builder temporaries */
    uint64_t host_bytes;             /* brick tables held on the host while building */
    uint64_t validate_samples, validate_mismatches;
} vrc_build_info;
int vrc_build_shell_terrain(vrc_caster *h, uint32_t depth, uint64_t seed, int32_t thickness, int32_t octave_floor,
                            uint32_t flags, uint64_t validate_samples, const int32_t *probe_xy, uint32_t n_probe,
                            int32_t *probe_lohi, vrc_build_info *info);
/* The same builder for ANY column scene: column (x,y) is solid for lo[x + dim*y] <= z <= hi[x + dim*y] (uint16[dim*dim]
 * each; lo == NULL: solid from z = 0 up).  This is Octree::Generate (src/map/Octree.cpp:13-43) for terrains -- e.g. the
 * reference's own diamond-square height field, Map::GenerateHeightBitmap (src/map/Map.cpp:144-262,
 * vrc_scene_diamond_square) -- without the dense char[D^3] grid: only the 2-D field crosses PCIe, the tree is built in
 * the handle's HBM and installed as the octree.  Bit-identical to vrc_octree_from_columns(..., VRC_LAYOUT_NO_PAGE_HEADERS).
 * validate_samples as above (tree point queries against the columns).                                               */
int vrc_build_heightfield(vrc_caster *h, uint32_t depth, const uint16_t *hi, const uint16_t *lo, uint32_t flags,
                          uint64_t validate_samples, vrc_build_info *info);
/* Host twin of vrc_build_heightfield (sequential emitter, depth <= 13): the array to compare the device build with. */
int vrc_octree_from_columns(uint32_t depth, const uint16_t *hi, const uint16_t *lo, uint32_t layout, uint64_t **descriptors,
                            uint64_t *n_descriptors, uint64_t *root_index);
/* The same builder for Octree::Generate's own input (src/map/Octree.cpp:13-43): a dense grid int8[dim^3],
 * x + dim*(y + dim*z), any non-zero voxel solid -- the reference's Map::data (src/map/Map.cpp:7-30).  The grid crosses
 * PCIe once; occupancy pyramid, count, emit and validate run in the handle's HBM and the tree is installed as the octree
 * (materials: flag VRC_BUILD_ATTACHMENTS turns the grid's values into the attachment arrays on the device -- one slot
 * per non-empty 2^3 block in grid order -- so the SVO branch renders the map's materials, mirrors included; without
 * the flag every voxel is material 5).  3 <= depth <= 12 (4096^3 = 64 GiB).
 * Bit-identical to vrc_octree_generate_ex(grid, dim, VRC_LAYOUT_NO_PAGE_HEADERS).  validate_samples: tree point queries
 * against the grid, half of them on / next to solid voxels.  grid == NULL: build from the map vrc_assign_map has already
 * put into this handle's HBM (it must be dim^3) -- a host that uses both branches, like the reference's Application,
 * uploads its Map once.                                                                                             */
int vrc_build_dense_grid(vrc_caster *h, uint32_t depth, const int8_t *grid, uint32_t flags, uint64_t validate_samples,
                         vrc_build_info *info);
/* Host twin: vrc_octree_generate with the layout flags of vrc_scene_shell_terrain_ex (array sized exactly). */
int vrc_octree_generate_ex(const int8_t *grid, uint32_t dim, uint32_t layout, uint64_t **descriptors,
                           uint64_t *n_descriptors, uint64_t *root_index);
/* Read descriptors [first, first + count) of the resident octree back to the host (tests, tools). */
int vrc_read_descriptors(vrc_caster *h, uint64_t first, uint64_t count, uint64_t *out);
int vrc_octree_size(vrc_caster *h, uint64_t *n_descriptors, uint64_t *root_index);
/* The materials of the resident octree, in the form vrc_assign_octree_attachments takes (tests, tools: an edited tree's exist only
 * on the device): *n_attachments receives the number of slots, 0 for a tree without materials; lookup (uint32[n_descriptors])
 * and attachments (uint64[capacity >= *n_attachments]) are filled where they are given.                                      */
int vrc_read_attachments(vrc_caster *h, uint32_t *lookup, uint64_t *attachments, uint64_t capacity, uint64_t *n_attachments);

/* Synthetic 256x256-style atlas: texel = hash(x,y) & 0xFFFFFF, alpha 255.    */
int vrc_scene_atlas(int32_t width, int32_t height, uint8_t *rgba8);

/* Octree::GetVoxel (src/map/Octree.cpp:45-158), the CPU twin of get_oct_vox
 * (kernels/ray_caster_kernel.cl:140-251), on a host copy of the array:
 * found, resolution and sub_oct_pos as that traversal leaves them.            */
int vrc_octree_get_voxel(const uint64_t *descriptors, uint64_t root_index, uint32_t dim,
                         const int32_t position[3], int32_t *found, int32_t *resolution,
                         int32_t sub_oct_pos[3]);

/* Octree::Load (declared, never defined: include/map/Octree.h:38) and its counterpart: a flat little-endian
 * file of the descriptor array (+ optional attachment buffers).  Loaded arrays are malloc'ed (vrc_free).      */
int vrc_octree_save(const char *path, uint32_t dim, const uint64_t *descriptors, uint64_t n_descriptors,
                    uint64_t root_index, const uint32_t *lookup, const uint64_t *attachments,
                    uint64_t n_attachments);
int vrc_octree_load(const char *path, uint32_t *dim, uint64_t **descriptors, uint64_t *n_descriptors,
                    uint64_t *root_index, uint32_t **lookup, uint64_t **attachments, uint64_t *n_attachments);

/* Streaming upload of a saved tree (a scene is built once, then streamed): reads the file written by
 * vrc_octree_save in chunks through pinned staging buffers straight into device memory (host memory use is two
 * chunks, whatever the size of the tree), installs the attachment buffers if the file has them, and sets the
 * octree_root_index setting like vrc_assign_octree (CLCaster.cpp:113).  *dim receives the map dimension the file
 * was saved with (the host still owns the octree_dimensions setting).                                            */
int vrc_assign_octree_file(vrc_caster *h, const char *path, uint32_t *dim);

void vrc_free(void *p);

#ifdef __cplusplus
}
#endif
#endif
