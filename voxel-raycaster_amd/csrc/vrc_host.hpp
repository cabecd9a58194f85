// vrc_host.hpp -- what the files of the host layer share (vrc_api.cpp: handles, settings, trees, groups and frames; vrc_query.cpp:
// the calls that read the resident scene; vrc_scene_edit.cpp: the calls that change it).  Internal: not installed, not part of
// include/vrc.h.  The helpers are defined in vrc_api.cpp, those from bind_scene to volume_check in vrc_query.cpp; they live in
// namespace vrc_host so that nothing collides with the C names.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <initializer_list>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/vrc.h"
#include "vrc_launch.h"
#include "vrc_params.h"
#ifdef VRC_INDEX_AUDIT
#include "index_audit.hpp"
#endif

namespace vrc_host {

// the caller's current device, put back on every path out of the scope (a group handle works on rank 0's GPU; a group that lets
// go of its peers' trees goes on allocating there)
struct DeviceRestore {
    int dev = -1;
    DeviceRestore() { if (hipGetDevice(&dev) != hipSuccess) { dev = -1; (void)hipGetLastError(); } }
    ~DeviceRestore() { if (dev >= 0) (void)hipSetDevice(dev); }
};

template <class T>
void release(T *&p) {
    if (p) { (void)hipFree(p); p = nullptr; }
}

// What a structure derived from a tree was built for, or failed to be built for: the table's level, the root, the tree's depth ...
struct TableKey {
    int log2 = 0; uint64_t root = 0; int depth = 0;
    bool operator==(const TableKey &o) const { return log2 == o.log2 && root == o.root && depth == o.depth; }
};
// ... and for the boxes their form (box_mode) and the levels and records asked for.  (A FAILURE is remembered without the last
// two: they stay 0 in its key.)
struct BoxKey {
    TableKey at; int mode = 0; int64_t levels_asked = 0, records_asked = 0;
    bool operator==(const BoxKey &o) const { return at == o.at && mode == o.mode && levels_asked == o.levels_asked && records_asked == o.records_asked; }
};
// An allocation failed: the frames go on without the structure.  Not retried every frame -- but retried as soon as what was
// asked for changes (level, root, depth) or the host sets coarse_log2 / empty_boxes again (vrc_setting_add / _set)
template <class Key>
struct Derived {
    Key built, failed;
    bool gave_up = false;
    std::string note;                                     // why (cleared when the structure is built after all)
};

}  // namespace vrc_host

using namespace vrc_host;       // (the structs below and both host files name these without the prefix)

struct vrc_setting { std::string name, define; int64_t value; };

// One descriptor array resident on one GPU, with its materials and with what the kernels derive from it (the dense table of
// the tree's top, the empty boxes).  Everything here is a function of the TREE, not of a caster: the handles that render the
// same array on the same GPU -- the ranks of a group that sit on rank 0's GPU, a handle that adopted another handle's tree
// (vrc_assign_octree_from) -- hold one Tree between them, so the 1 GB table and the boxes exist once.  The reference never
// frees or shares anything (CLCaster.cpp:5-12); this is footprint hygiene for trees of BASELINE configs[4]'s size.
struct vrc_tree {
    int device = 0;
    uint64_t *d_desc = nullptr; uint64_t n_desc = 0;
    uint32_t *d_attach_lookup = nullptr; uint64_t *d_attach = nullptr; uint64_t n_attach = 0;
    // words allocated, once an edit (vrc_set_voxels) has grown an array beyond what it holds; 0: exactly what it holds
    uint64_t cap_desc = 0, cap_lookup = 0, cap_attach = 0;
    uint64_t desc_capacity() const { return cap_desc ? cap_desc : n_desc; }
    uint64_t lookup_capacity() const { return cap_lookup ? cap_lookup : n_desc; }
    uint64_t attach_capacity() const { return cap_attach ? cap_attach : std::max<uint64_t>(n_attach, 1); }
    // derived, built on first use by whichever handle needs them first (guard: handles of several host threads)
    std::mutex guard;
    uint64_t *d_coarse = nullptr; Derived<TableKey> coarse;
    uint32_t *d_boxes = nullptr, *d_box_aux = nullptr; Derived<BoxKey> boxes; double box_build_seconds = 0.0;
    unsigned long long box_queries_cut = 0;               // region queries of the build that gave up at their budget (boxes smaller than they could be)
    // box records: one per descriptor (box_mode 1: record = descriptor index) or for the upper levels only (box_mode 2: breadth-first
    // records, d_box_child = first-child record, d_box_desc / d_box_pos = descriptor and position of a record, kept for the self-check)
    int box_levels = 0; uint64_t box_records = 0;
    uint32_t *d_box_child = nullptr; uint64_t *d_box_desc = nullptr, *d_box_pos = nullptr;
    ~vrc_tree() {
        {
            DeviceRestore restore;
            (void)hipSetDevice(device);
            release(d_coarse); release(d_boxes); release(d_box_aux); release(d_box_child); release(d_box_desc); release(d_box_pos);
            release(d_desc); release(d_attach_lookup); release(d_attach);
        }
        (void)hipGetLastError();
    }
};

struct vrc_caster {
    int device = 0;
    hipStream_t stream = nullptr;
    std::string error;

    // scene buffers (device)
    int8_t *d_map = nullptr; int32_t map_dim[3] = {0, 0, 0};
    // the tree (shared, see vrc_tree), attached only once it is complete: "has an octree" is tree != nullptr
    std::shared_ptr<vrc_tree> tree;
    bool owns_desc = true;                // false: the tree is another handle's too (a group rank on rank 0's GPU, vrc_assign_octree_from)
    bool own_copy = false;                // group flag VRC_GROUP_OWN_COPIES: never share, always take the device-to-device copy path
    int32_t peer_access = -1;             // -1 same GPU as rank 0 / rank 0 itself, 1 direct peer access enabled, 0 the runtime stages the copies
    void *pinned_stage = nullptr; size_t pinned_stage_bytes = 0;   // read-back staging for a pageable destination (groups)
    bool last_frame_boxes = false;        // the last enqueued frame was rendered with the tree's empty boxes (its descriptor-read counts are the box traversal's)
    vrc::LaunchRecord last_launch = {};   // the kernel instance the last enqueued frame was launched with (vrc_last_kernel)
    bool last_frame_wrote_hits = false;   // d_hits belongs to the last enqueued frame (setting hit_records was on)
    float *d_viewport = nullptr; float *d_image = nullptr; int32_t *d_hits = nullptr; uint8_t *d_rgba8 = nullptr;
    uint32_t *d_jump_cache = nullptr, *d_jump_slots = nullptr; int jump_slot_count = 0, jump_slot_threads = 0;   // Euclid tables of the exact closed-form jumps (exact_jump.hpp), per resident block
    int32_t width = 0, height = 0;
    bool sliced = false;                  // viewport / image / hits hold only this rank's rows
    int32_t buffer_rows = 0;              // rows the three buffers hold
    uint8_t *d_atlas = nullptr; int32_t atlas_w = 0, atlas_h = 0, tile_w = 0, tile_h = 0;
    unsigned long long *d_partials = nullptr; int partial_blocks = 0;
    unsigned long long *d_counters = nullptr;
    int32_t *d_frame = nullptr;           // {bias[3], reads}
    unsigned int *wd_flag = nullptr;      // host-mapped: raised by the kernel's round watchdog
    float *d_query_rays = nullptr; int32_t *d_query_out = nullptr; int64_t query_capacity = 0;   // vrc_cast_rays' staging (rays)
    // vrc_box_intersection: staging of the host call (boxes, records, counts, list), per-box and per-item scratch, scan storage
    float *d_box_in = nullptr; int32_t *d_box_rec = nullptr; int64_t *d_box_cnt = nullptr; int64_t box_io_capacity = 0;
    int32_t *d_box_vox = nullptr; size_t box_vox_bytes = 0;
    void *d_box_plan = nullptr; int64_t *d_box_scan = nullptr; int32_t *d_box_corner = nullptr; int64_t box_capacity = 0;
    int64_t *d_box_items = nullptr; int64_t box_item_capacity = 0;
    void *d_box_temp = nullptr; size_t box_temp_bytes = 0;
    // vrc_sweep_boxes: staging of the host call (sweeps, records); the start test's records, counts and first voxels, the
    // shape flags and their scan; the number of wave-shaped sweeps (read back with the start test's item totals)
    float *d_sweep_in = nullptr; int32_t *d_sweep_out = nullptr; int64_t sweep_io_capacity = 0;
    int32_t *d_sweep_rec = nullptr, *d_sweep_vox = nullptr; int64_t *d_sweep_cnt = nullptr, *d_sweep_scan = nullptr; int64_t sweep_capacity = 0;
    int64_t sweep_n_big = 0;
    // vrc_get_voxels / vrc_read_regions: staging of the host calls (positions or corners in, values or bytes out)
    int32_t *d_read_in = nullptr; int64_t read_in_capacity = 0;
    void *d_read_out = nullptr; size_t read_out_bytes = 0;
    // vrc_extract_faces: the faces per (region, brick), their scan and the host call's counts (its corners and its list stage through
    // d_read_in / d_read_out, the scan's storage is d_box_temp)
    int64_t *d_face_items = nullptr; int64_t face_item_capacity = 0;
    // the scene edits (vrc_scene_edit.cpp).  d_edit_in: no longer used, every edit stages through d_region_in; the field stays until the
    // scratch gets an owner of its own ("Left out").  Keys and edit numbers (unsorted, sorted), the unique keys
    // and their run lengths; the counters; rocprim's storage; the touched nodes above the bricks (keys) and every touched node's record
    int32_t *d_edit_in = nullptr; int64_t edit_in_capacity = 0;
    uint64_t *d_edit_keys = nullptr, *d_edit_unique = nullptr; uint32_t *d_edit_order = nullptr, *d_edit_counts = nullptr; int64_t edit_capacity = 0;
    unsigned long long *d_edit_counters = nullptr;
    void *d_edit_temp = nullptr; size_t edit_temp_bytes = 0;
    uint64_t *d_edit_levels = nullptr; int64_t edit_level_capacity = 0;
    uint32_t *d_edit_rec_masks = nullptr; uint64_t *d_edit_rec_child = nullptr; int64_t edit_rec_capacity = 0;
    // staging of a host call (its first array, then the second at a 16-byte-aligned offset); the region edits' bricks per
    // operation and their scan.  Everything behind the pairs is the edit's own scratch above.
    void *d_region_in = nullptr; size_t region_in_bytes = 0;
    uint64_t *d_region_counts = nullptr; int64_t region_capacity = 0;

    // live (retained) host pointers
    const float *cam_dir = nullptr, *cam_pos = nullptr;
    const float *cam_trig = nullptr;      // vrc_assign_camera_trig: the host's own sin / cos of the two angles (nullptr: sinf / cosf here)
    const float *lights = nullptr; const int32_t *light_count = nullptr;

    std::vector<vrc_setting> settings;    // <= 64 slots (include/CLCaster.h:303)

    int32_t tile_rank = 0, tile_world = 1, band_rows = 8;
    bool validated = false;
    int last_blocks = 0;
    uint64_t frames_enqueued = 0;
    uint64_t sched_stats[8] = {0, 0, 0, 0, 0, 0, 0, 0};

    // kernel timing
    struct EvPair { hipEvent_t a, b; };
    std::vector<EvPair> pending, pool;
    uint64_t timed_launches = 0; double timed_ms = 0.0;

    // group: this handle is rank 0, peers are ranks 1..n-1
    std::vector<vrc_caster *> peers;
    bool is_peer = false;
};

namespace vrc_host {

int fail(vrc_caster *h, int code, const char *fmt, ...);

#define HIP_TRY(h, call)                                                                          \
    do {                                                                                          \
        hipError_t e_ = (call);                                                                   \
        if (e_ != hipSuccess) {                                                                   \
            (void)hipGetLastError();      /* reported here: not left behind for a later launch check */ \
            return fail(h, e_ == hipErrorOutOfMemory ? VRC_ERR_OUT_OF_MEMORY : VRC_ERR_DEVICE,    \
                        "%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, __LINE__); \
        }                                                                                         \
    } while (0)

// a step that reports through the handle's own error text: its failure is the caller's
#define VRC_TRY(...)                                                                              \
    do {                                                                                          \
        const int rc_ = (__VA_ARGS__);                                                            \
        if (rc_ != VRC_OK) return rc_;                                                            \
    } while (0)

// replicate a call on every other rank of a group; the first failure is reported through rank 0
#define FOR_PEERS(h, expr)                                                                        \
    do {                                                                                          \
        for (size_t pi_ = 0; pi_ < (h)->peers.size(); pi_++) {                                    \
            vrc_caster *q = (h)->peers[pi_];                                                      \
            const int rc_ = (expr);                                                               \
            if (rc_ != VRC_OK) return fail(h, rc_, "rank %zu: %s", pi_ + 1, q->error.c_str());    \
        }                                                                                         \
    } while (0)

int64_t setting_or(const vrc_caster *h, const char *name, int64_t dflt);
int set_setting(vrc_caster *h, const char *name, const char *define, int64_t value);
int log2_exact(int64_t v);
// the tree's empty boxes, in either form
void release_boxes(vrc_tree *t);
// materials are bound as a pair or not at all (the frame's RaycastParams and the queries' SceneView); the caller holds t->guard
void bind_attachments(const vrc_tree *t, const uint32_t *&attach_lookup, const uint64_t *&attachments);
// The scene a query runs against (the SceneView of QueryParams, BoxParams and ReadParams), from the handle's settings and its
// tree.  The caller holds t->guard.
void bind_scene(const vrc_caster *h, const vrc_tree *t, vrc::SceneView &q);
// the argument and readiness checks the queries share; nothing is launched when one fails
int query_check(vrc_caster *h, const void *rays, int64_t n, int32_t max_steps, uint32_t flags, const void *out, const char *what);
// device pointers the kernel may dereference: memory of the handle's GPU, managed memory or page-locked host memory
bool query_pointer_ok(const vrc_caster *h, const void *p);
// work the host queued on the null stream (a torch tensor's fill, say) comes first: the handle's stream does not wait for it by itself
int wait_for_null_stream(vrc_caster *h);
// size[] of the region reads and of the pastes: given, and every edge at least 1 ...
int size_check(vrc_caster *h, const int32_t size[3], const char *what);
// ... and their n regions of V = size[0] size[1] size[2] bytes each (n >= 0): *total = n V, which the `holder` (the output, the
// data) of n_bytes must have room for.  A caller that wants V itself (volume != nullptr) is told apart which product overflowed.
int volume_check(vrc_caster *h, int64_t n, const int32_t size[3], size_t n_bytes, const char *holder, uint64_t *volume, size_t *total, const char *what);

// Grow device buffers that share one capacity (staging and scratch grow on demand; freed by the release_* calls, destroy).  A frame
// in flight must not lose buffers it does not use anyway: the stream is drained first.
struct GrowBuffer {
    void **p; size_t bytes;
    template <class T> GrowBuffer(T *&ptr, size_t n) : p((void **)&ptr), bytes(n) {}
};
template <class Cap>
int grow(vrc_caster *h, Cap &have, Cap want, std::initializer_list<GrowBuffer> buffers) {
    if (have >= want) return VRC_OK;
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    for (const GrowBuffer &b : buffers)
        if (*b.p) { (void)hipFree(*b.p); *b.p = nullptr; }
    have = 0;
    for (const GrowBuffer &b : buffers) HIP_TRY(h, hipMalloc(b.p, b.bytes));
    have = want;
    return VRC_OK;
}

// A size-versioned struct goes back to the caller (vrc_memory2, vrc_edit_info, vrc_compact_info): never more than the caller's own
// struct holds, and its struct_size says how much that was
template <class Info>
void write_info(Info *info, Info &out) {
    const uint32_t bytes = std::min<uint32_t>(info->struct_size, (uint32_t)sizeof(out));
    out.struct_size = bytes;
    memcpy(info, &out, bytes);
}

// The kernels of a call run in segments on the handle's stream; the device time of each, between two events, is added to *seconds.
struct SegmentTimer {
    hipEvent_t a = nullptr, b = nullptr;
    hipStream_t stream = nullptr; double *seconds = nullptr;
    ~SegmentTimer() { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); }
    hipError_t init(hipStream_t s, double *sum) { stream = s; seconds = sum; hipError_t e = hipEventCreate(&a); return e == hipSuccess ? hipEventCreate(&b) : e; }
    hipError_t start() { return hipEventRecord(a, stream); }
    // the segment's last kernel is in the stream: what the caller enqueues between here and wait() (a read-back) is not timed
    hipError_t stop() { return hipEventRecord(b, stream); }
    hipError_t wait() {
        float ms = 0.f;
        const hipError_t e = hipStreamSynchronize(stream);
        if (e == hipSuccess && hipEventElapsedTime(&ms, a, b) == hipSuccess) *seconds += ms * 1e-3; else (void)hipGetLastError();
        return e;
    }
    // stop, the read-back that sizes the next segment (if any), wait
    hipError_t end(void *host = nullptr, const void *dev = nullptr, size_t bytes = 0) {
        hipError_t e = stop();
        if (e == hipSuccess && host) e = hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, stream);
        return e == hipSuccess ? wait() : e;
    }
};

#ifdef VRC_INDEX_AUDIT
// The index-audit build (index_audit.hpp): the extents of the arrays the kernels index, published to the device table of every .hip
// file from the variables the allocations were made with.  The tables are process-global and per device, so the audit build
// serialises: the device is drained before the extents change, and the report drains it before it reads.  One host thread.  The
// host keeps ONE current set of extents and every publish writes all of it to the device that is current, so the ranks of a group on
// several devices each get the whole set at their own launches; the shrink knob applies to every device alike.
// (every launch site sets ALL the arrays its kernels may index; what it does not set keeps the extent of the launch before, which those
// kernels never look at)
extern unsigned long long g_audit_shrink[vrc::audit::kArrayCount];       // test-only: taken off the extent of that array (vrc_index_audit_shrink)
extern unsigned long long g_audit_current[vrc::audit::kArrayCount];      // extent + 1 as published last; 0: never (counted, not checked)
struct AuditExtents {
    unsigned long long e1[vrc::audit::kArrayCount];
    AuditExtents() { memcpy(e1, g_audit_current, sizeof(e1)); }
    void set(int id, unsigned long long extent) {
        const unsigned long long cut = g_audit_shrink[id];
        e1[id] = (extent > cut ? extent - cut : 0) + 1;
    }
};
hipError_t audit_publish(const AuditExtents &x);
// the tree's arrays and what is derived from it
void audit_tree(AuditExtents &x, const vrc_tree *t);
#define VRC_AUDIT_PUBLISH(h, x) HIP_TRY(h, audit_publish(x))
#endif

}  // namespace vrc_host
