// vrc_query.cpp -- the calls of include/vrc.h that read the resident scene: ray queries (vrc_cast_rays, raycast_query.hip), box
// queries (vrc_box_intersection, box_query.hip), swept boxes (vrc_sweep_boxes, box_sweep.hip), voxel reads (vrc_get_voxels /
// vrc_read_regions, voxel_read.hip) and the exposed faces (vrc_extract_faces, face_extract.hip), with their _device variants; and
// the checks and the scene binding the scene edits share with them (vrc_host.hpp).
//
// They are one procedure.  The call checks its arguments and the handle's readiness (query_check last) and returns at n == 0;
// nothing has touched the device by then.  A host call (host_call) switches to the handle's GPU, stages its arrays down, enqueues,
// stages the results up and waits for the stream.  A _device call (device_call) checks the alignment of its arrays, switches,
// checks that the GPU can reach them, lets the null stream's work go first, enqueues on the caller's arrays and waits.  The
// enqueue step takes the tree's guard and holds it until its last kernel is in the stream, as a frame does -- the faces, which
// wait for their total in between, until the list is written.  A query never builds a derived structure: it uses the coarse
// table and the empty boxes that vrc_prepare / validate / a frame has built for the tree, and does without them otherwise.
#include "box_query.h"
#include "box_sweep.h"
#include "face_extract.h"
#include "raycast_query.h"
#include "voxel_read.h"
#include "vrc_host.hpp"

// ---------------------------------------------------------------------------------------------------------------------------
// what every family shares, the scene edits too
// ---------------------------------------------------------------------------------------------------------------------------
namespace {

int flags_check(vrc_caster *h, uint32_t flags, uint32_t known, const char *what) {
    if (flags & ~known) return fail(h, VRC_ERR_INVALID_ARGUMENT, "%s: unknown flag bits 0x%x", what, (unsigned)(flags & ~known));
    return VRC_OK;
}

// The tree's table and boxes, if they were built for this root and depth.  The caller holds t->guard.
bool coarse_for(const vrc_tree *t, uint64_t root, int n) {
    const TableKey &k = t->coarse.built;
    return t->d_coarse && k.root == root && k.depth == n && k.log2 >= 1 && k.log2 <= n - 2;
}
bool boxes_for(const vrc_tree *t, uint64_t root, int n) {
    return coarse_for(t, root, n) && t->d_boxes && t->d_box_aux && t->boxes.built.at == t->coarse.built;
}

}  // namespace

// the argument and readiness checks every query and edit shares; nothing is launched when one fails
int vrc_host::query_check(vrc_caster *h, const void *rays, int64_t n, int32_t max_steps, uint32_t flags, const void *out, const char *what) {
    if (n < 0) return fail(h, VRC_ERR_INVALID_ARGUMENT, "%s: n = %lld < 0", what, (long long)n);
    if (max_steps < 0) return fail(h, VRC_ERR_INVALID_ARGUMENT, "%s: max_steps = %d < 0", what, (int)max_steps);
    VRC_TRY(flags_check(h, flags, VRC_RAY_AS_PIXEL, what));
    if (n > 0 && (!rays || !out)) return fail(h, VRC_ERR_INVALID_ARGUMENT, "%s: null rays or output", what);
    if (!h->validated) return fail(h, VRC_ERR_NOT_READY, "%s: validate() has not succeeded", what);
    if (!h->tree) return fail(h, VRC_ERR_NOT_READY, "%s: no octree assigned", what);
    const int n2 = log2_exact(setting_or(h, "octree_dimensions", 0));
    if (n2 < 1 || n2 > vrc::kMaxLevels) return fail(h, VRC_ERR_INVALID_ARGUMENT, "%s: octree_dimensions must be a power of two in [2, 2^%d]", what, vrc::kMaxLevels);
    const int64_t root = setting_or(h, "octree_root_index", 0);
    if (root < 0 || (uint64_t)root >= h->tree->n_desc) return fail(h, VRC_ERR_INVALID_ARGUMENT, "%s: octree_root_index out of range", what);
    if (setting_or(h, "using_octree", 0) != 0 && !h->d_map) return fail(h, VRC_ERR_NOT_READY, "%s: dense map not assigned (using_octree != 0 selects the array branch)", what);
    return VRC_OK;
}

bool vrc_host::query_pointer_ok(const vrc_caster *h, const void *p) {
    hipPointerAttribute_t a;
    memset(&a, 0, sizeof(a));
    const hipError_t e = hipPointerGetAttributes(&a, p);
    (void)hipGetLastError();
    if (e != hipSuccess) return false;
    if (a.type == hipMemoryTypeDevice || a.type == hipMemoryTypeArray) return a.device == h->device;
    return a.type == hipMemoryTypeHost || a.type == hipMemoryTypeManaged || a.type == hipMemoryTypeUnified;
}

int vrc_host::wait_for_null_stream(vrc_caster *h) {
    hipEvent_t ready = nullptr;
    HIP_TRY(h, hipEventCreateWithFlags(&ready, hipEventDisableTiming));
    hipError_t e = hipEventRecord(ready, nullptr);
    if (e == hipSuccess) e = hipStreamWaitEvent(h->stream, ready, 0);
    (void)hipEventDestroy(ready);
    HIP_TRY(h, e);
    return VRC_OK;
}

int vrc_host::size_check(vrc_caster *h, const int32_t size[3], const char *what) {
    if (!size) return fail(h, VRC_ERR_INVALID_ARGUMENT, "%s: null size", what);
    for (int a = 0; a < 3; a++)
        if (size[a] < 1) return fail(h, VRC_ERR_INVALID_ARGUMENT, "%s: size[%d] = %d < 1", what, a, (int)size[a]);
    return VRC_OK;
}

int vrc_host::volume_check(vrc_caster *h, int64_t n, const int32_t size[3], size_t n_bytes, const char *holder, uint64_t *volume, size_t *total,
                           const char *what) {
    size_t bytes = (size_t)size[0];
    for (uint64_t f : {(uint64_t)size[1], (uint64_t)size[2]}) {
        if (bytes > SIZE_MAX / f) return fail(h, VRC_ERR_LIMIT, "%s: %ssize[0] * size[1] * size[2] bytes overflows size_t", what, volume ? "" : "n * ");
        bytes *= (size_t)f;
    }
    if (volume) *volume = bytes;
    if (n > 0 && bytes > SIZE_MAX / (uint64_t)n) return fail(h, VRC_ERR_LIMIT, "%s: n * size[0] * size[1] * size[2] bytes overflows size_t", what);
    bytes *= (size_t)n;
    if (bytes > (size_t)INT64_MAX) return fail(h, VRC_ERR_LIMIT, "%s: more than 2^63 bytes", what);      // (the kernels count their waves in int64)
    if (n_bytes < bytes) return fail(h, VRC_ERR_INVALID_ARGUMENT, "%s: %s holds %zu bytes, the regions need %zu", what, holder, n_bytes, bytes);
    *total = bytes;
    return VRC_OK;
}

void vrc_host::bind_scene(const vrc_caster *h, const vrc_tree *t, vrc::SceneView &q) {
    q.svo = setting_or(h, "using_octree", 0) == 0 ? 1 : 0;
    q.descriptors = t->d_desc;
    q.root_index = (uint64_t)setting_or(h, "octree_root_index", 0);
    q.log2_dim = log2_exact(setting_or(h, "octree_dimensions", 0));
    if (q.svo) {
        q.map_dim[0] = q.map_dim[1] = q.map_dim[2] = 1 << q.log2_dim;
        bind_attachments(t, q.attach_lookup, q.attachments);
        if (setting_or(h, "coarse_log2", -1) != 0 && coarse_for(t, q.root_index, q.log2_dim)) { q.coarse = t->d_coarse; q.coarse_log2 = t->coarse.built.log2; }
    } else {
        for (int a = 0; a < 3; a++) q.map_dim[a] = h->map_dim[a];
        q.map = h->d_map;
        q.map_bytes = (uint64_t)h->map_dim[0] * (uint64_t)h->map_dim[1] * (uint64_t)h->map_dim[2];
    }
#ifdef VRC_INDEX_AUDIT
    {   // the tree reads of the query, box, sweep and voxel-read kernels (svo_node.hpp); a failure shows as unpublished extents
        AuditExtents x;
        audit_tree(x, t);
        x.set(vrc::audit::kMap, h->d_map ? (size_t)h->map_dim[0] * h->map_dim[1] * h->map_dim[2] : 0);
        if (audit_publish(x) != hipSuccess) {              // never run a query against another launch's extents: none, then (counted, not checked)
            (void)hipGetLastError();
            memset(x.e1, 0, sizeof(x.e1));
            (void)audit_publish(x);
        }
    }
#endif
}

namespace {

// The host call, after its checks: `work` stages the arrays down, enqueues and stages the results up, all on the handle's stream
// (current device: h->device), which is waited for here.  The caller's device is put back.
template <class Work>
int host_call(vrc_caster *h, Work work) {
    DeviceRestore restore;
    HIP_TRY(h, hipSetDevice(h->device));
    VRC_TRY(work());
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return VRC_OK;
}

// one array of a _device call: where it is, the alignment its elements need (a mask), and whether this call touches it at all
struct DeviceArray { const void *p; uintptr_t mask; bool used = true; };

// The _device call, after its checks: `aligned` is what it says of a misaligned array, `reachable` names the arrays the GPU
// cannot reach; `work` enqueues on the handle's stream, which has waited for the null stream's work and is waited for here.
template <class Work>
int device_call(vrc_caster *h, std::initializer_list<DeviceArray> arrays, const char *what, const char *aligned, const char *reachable, Work work) {
    for (const DeviceArray &a : arrays)
        if (a.used && ((uintptr_t)a.p & a.mask)) return fail(h, VRC_ERR_INVALID_ARGUMENT, "%s: %s", what, aligned);
    DeviceRestore restore;
    HIP_TRY(h, hipSetDevice(h->device));
    for (const DeviceArray &a : arrays)
        if (a.used && !query_pointer_ok(h, a.p))
            return fail(h, VRC_ERR_INVALID_ARGUMENT, "%s: %s must be memory the GPU of the handle (device %d) can read and write", what, reachable, h->device);
    VRC_TRY(wait_for_null_stream(h));
    VRC_TRY(work());
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return VRC_OK;
}

// the bricks a region of this many voxels along an axis touches there at most, whatever its alignment
int64_t bricks_along(int32_t size) { return ((int64_t)size + 6) / 8 + 1; }

// ---------------------------------------------------------------------------------------------------------------------------
// batched ray queries (vrc_cast_rays / vrc_cast_rays_device, raycast_query.hip)
// ---------------------------------------------------------------------------------------------------------------------------
// One launch on the handle's stream (current device: h->device).  The tree's guard is held until the kernel is enqueued, as a
// frame holds it.
int query_enqueue(vrc_caster *h, const float *d_rays, int64_t n, int32_t max_steps, uint32_t flags, int32_t *d_out) {
    vrc_tree *t = h->tree.get();
    std::unique_lock<std::mutex> lock(t->guard);
    vrc::QueryParams q;
    memset(&q, 0, sizeof(q));
    q.rays = d_rays; q.out = d_out; q.n = n; q.flags = flags;
    q.octree_bias = (int32_t)setting_or(h, "octree_bias", 1);
    bind_scene(h, t, q.scene);
    // max_steps = 0: no cap below the map's edge -- every iteration steps an axis, so 3 dim + 3 bounds a ray that starts inside
    const int64_t dim_max = std::max(q.scene.map_dim[0], std::max(q.scene.map_dim[1], q.scene.map_dim[2]));
    q.cap = max_steps > 0 ? max_steps : (int32_t)std::min<int64_t>(INT32_MAX, 3 * dim_max + 3);
    if (q.scene.coarse && setting_or(h, "empty_boxes", -1) != 0 && boxes_for(t, q.scene.root_index, q.scene.log2_dim)) {
        q.boxes = t->d_boxes; q.box_aux = t->d_box_aux; q.box_child = t->d_box_child; q.box_levels = t->box_levels;
    }
    HIP_TRY(h, vrc::launch_raycast_query(q, h->stream));
    return VRC_OK;
}

}  // namespace

extern "C" {

int vrc_cast_rays(vrc_caster *h, const float *rays, int64_t n, int32_t max_steps, uint32_t flags, int32_t *out) {
    if (!h) return VRC_ERR_INVALID_ARGUMENT;
    int rc = query_check(h, rays, n, max_steps, flags, out, "cast_rays");
    if (rc != VRC_OK || n == 0) return rc;
    return host_call(h, [&]() -> int {
        VRC_TRY(grow(h, h->query_capacity, n, {{h->d_query_rays, sizeof(float) * 6 * (size_t)n}, {h->d_query_out, sizeof(int32_t) * 8 * (size_t)n}}));
        HIP_TRY(h, hipMemcpyAsync(h->d_query_rays, rays, sizeof(float) * 6 * (size_t)n, hipMemcpyHostToDevice, h->stream));
        VRC_TRY(query_enqueue(h, h->d_query_rays, n, max_steps, flags, h->d_query_out));
        HIP_TRY(h, hipMemcpyAsync(out, h->d_query_out, sizeof(int32_t) * 8 * (size_t)n, hipMemcpyDeviceToHost, h->stream));
        return VRC_OK;
    });
}

int vrc_cast_rays_device(vrc_caster *h, const void *d_rays, int64_t n, int32_t max_steps, uint32_t flags, void *d_out) {
    if (!h) return VRC_ERR_INVALID_ARGUMENT;
    int rc = query_check(h, d_rays, n, max_steps, flags, d_out, "cast_rays_device");
    if (rc != VRC_OK || n == 0) return rc;
    return device_call(h, {{d_rays, 3u}, {d_out, 3u}}, "cast_rays_device", "rays and output must be 4-byte aligned", "rays and output",
                       [&] { return query_enqueue(h, static_cast<const float *>(d_rays), n, max_steps, flags, static_cast<int32_t *>(d_out)); });
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------------------------------------
// batched box-overlap queries (vrc_box_intersection / vrc_box_intersection_device, box_query.hip)
// ---------------------------------------------------------------------------------------------------------------------------
namespace {

// the argument checks of both calls, then the readiness checks of the ray queries; nothing is launched when one fails
int box_check(vrc_caster *h, const void *boxes, int64_t n, int32_t max_voxels, uint32_t flags, const void *records, const void *counts,
              const void *voxels, const char *what) {
    if (n < 0) return fail(h, VRC_ERR_INVALID_ARGUMENT, "%s: n = %lld < 0", what, (long long)n);
    if (max_voxels < 0) return fail(h, VRC_ERR_INVALID_ARGUMENT, "%s: max_voxels = %d < 0", what, (int)max_voxels);
    VRC_TRY(flags_check(h, flags, VRC_BOX_STOPPING_ONLY, what));
    if (n > 0 && (!boxes || !records || !counts)) return fail(h, VRC_ERR_INVALID_ARGUMENT, "%s: null boxes, records or counts", what);
    if (n > 0 && max_voxels > 0 && !voxels) return fail(h, VRC_ERR_INVALID_ARGUMENT, "%s: null voxels with max_voxels = %d", what, (int)max_voxels);
    if (max_voxels > 0 && (uint64_t)n > SIZE_MAX / 16u / (uint64_t)max_voxels)
        return fail(h, VRC_ERR_LIMIT, "%s: n * max_voxels * 16 bytes overflows size_t", what);
    return query_check(h, boxes, n, 0, 0, records, what);
}

// Plan, scans, count, (scan, emit), finalize on the handle's stream (current device: h->device) for the boxes, outputs and
// scene q names; the scratch fields of q are filled in here.  The caller holds the tree's guard.  One host wait in the middle:
// the item totals size the grid and the per-item scratch.
int box_passes(vrc_caster *h, vrc::BoxParams &q) {
    const int64_t n = q.n;
    const int32_t max_voxels = q.max_voxels;
    // the aligned space the items tile: the tree's, or the map's largest side rounded up
    const int32_t side = std::max(q.scene.map_dim[0], std::max(q.scene.map_dim[1], q.scene.map_dim[2]));
    q.space_log2 = 1;
    while ((1 << q.space_log2) < side) q.space_log2++;
    // per-box scratch: plan, the two item counts and their scans, the totals, the corners
    VRC_TRY(grow(h, h->box_capacity, n, {{h->d_box_plan, sizeof(vrc::BoxPlan) * (size_t)n}, {h->d_box_scan, sizeof(int64_t) * 5 * (size_t)n},
                                         {h->d_box_corner, sizeof(int32_t) * 6 * (size_t)n}}));
    int64_t *small_cnt = h->d_box_scan, *big_cnt = h->d_box_scan + n;
    q.plan = static_cast<vrc::BoxPlan *>(h->d_box_plan);
    q.small_end = h->d_box_scan + 2 * n; q.big_end = h->d_box_scan + 3 * n; q.acc_count = h->d_box_scan + 4 * n;
    q.acc_corner = h->d_box_corner;
    size_t need = 0;
    HIP_TRY(h, vrc::box_scan(nullptr, &need, small_cnt, q.small_end, n, h->stream));
    VRC_TRY(grow(h, h->box_temp_bytes, need, {{h->d_box_temp, need}}));
    HIP_TRY(h, vrc::launch_box_plan(q, small_cnt, big_cnt, h->stream));
    size_t bytes = h->box_temp_bytes;
    HIP_TRY(h, vrc::box_scan(h->d_box_temp, &bytes, small_cnt, q.small_end, n, h->stream));
    bytes = h->box_temp_bytes;
    HIP_TRY(h, vrc::box_scan(h->d_box_temp, &bytes, big_cnt, q.big_end, n, h->stream));
    int64_t totals[2] = {0, 0};
    HIP_TRY(h, hipMemcpyAsync(&totals[0], q.small_end + n - 1, sizeof(int64_t), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipMemcpyAsync(&totals[1], q.big_end + n - 1, sizeof(int64_t), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    q.n_small = totals[0]; q.n_big = totals[1];
    const int64_t items = q.n_small + q.n_big;
    const bool emit = max_voxels > 0 && items > 0;
    if (emit) {
        // per-item counts and their scan (an item's list offset inside its box)
        VRC_TRY(grow(h, h->box_item_capacity, items, {{h->d_box_items, sizeof(int64_t) * 2 * (size_t)items}}));
        q.item_count = h->d_box_items; q.item_end = h->d_box_items + items;
        need = 0;
        HIP_TRY(h, vrc::box_scan(nullptr, &need, q.item_count, q.item_end, items, h->stream));
        VRC_TRY(grow(h, h->box_temp_bytes, need, {{h->d_box_temp, need}}));
    }
    HIP_TRY(h, vrc::launch_box_count(q, 0, h->stream));
    if (emit) {
        bytes = h->box_temp_bytes;
        HIP_TRY(h, vrc::box_scan(h->d_box_temp, &bytes, q.item_count, q.item_end, items, h->stream));
        HIP_TRY(h, vrc::launch_box_count(q, 1, h->stream));
    }
    HIP_TRY(h, vrc::launch_box_finalize(q, h->stream));
    return VRC_OK;
}

// The tree's guard is held throughout, as query_enqueue holds it.
int box_enqueue(vrc_caster *h, const float *d_boxes, int64_t n, int32_t max_voxels, uint32_t flags, int32_t *d_rec, int64_t *d_cnt,
                int32_t *d_vox) {
    std::unique_lock<std::mutex> lock(h->tree->guard);
    vrc::BoxParams q;
    memset(&q, 0, sizeof(q));
    q.boxes = d_boxes; q.box_stride = 6; q.n = n; q.max_voxels = max_voxels; q.flags = flags;
    q.records = d_rec; q.counts = d_cnt; q.voxels = max_voxels > 0 ? d_vox : nullptr;
    bind_scene(h, h->tree.get(), q.scene);
    return box_passes(h, q);
}

}  // namespace

extern "C" {

int vrc_box_intersection(vrc_caster *h, const float *boxes, int64_t n, int32_t max_voxels, uint32_t flags, int32_t *records,
                         int64_t *counts, int32_t *voxels) {
    if (!h) return VRC_ERR_INVALID_ARGUMENT;
    int rc = box_check(h, boxes, n, max_voxels, flags, records, counts, voxels, "box_intersection");
    if (rc != VRC_OK || n == 0) return rc;
    return host_call(h, [&]() -> int {
        VRC_TRY(grow(h, h->box_io_capacity, n, {{h->d_box_in, sizeof(float) * 6 * (size_t)n}, {h->d_box_rec, sizeof(int32_t) * 8 * (size_t)n},
                                            {h->d_box_cnt, sizeof(int64_t) * (size_t)n}}));
        const size_t vox_bytes = (size_t)n * (size_t)max_voxels * 16u;
        if (vox_bytes) VRC_TRY(grow(h, h->box_vox_bytes, vox_bytes, {{h->d_box_vox, vox_bytes}}));
        HIP_TRY(h, hipMemcpyAsync(h->d_box_in, boxes, sizeof(float) * 6 * (size_t)n, hipMemcpyHostToDevice, h->stream));
        // the list goes down first: the entries a box does not write come back as the caller left them
        if (vox_bytes) HIP_TRY(h, hipMemcpyAsync(h->d_box_vox, voxels, vox_bytes, hipMemcpyHostToDevice, h->stream));
        VRC_TRY(box_enqueue(h, h->d_box_in, n, max_voxels, flags, h->d_box_rec, h->d_box_cnt, h->d_box_vox));
        HIP_TRY(h, hipMemcpyAsync(records, h->d_box_rec, sizeof(int32_t) * 8 * (size_t)n, hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(h, hipMemcpyAsync(counts, h->d_box_cnt, sizeof(int64_t) * (size_t)n, hipMemcpyDeviceToHost, h->stream));
        if (vox_bytes) HIP_TRY(h, hipMemcpyAsync(voxels, h->d_box_vox, vox_bytes, hipMemcpyDeviceToHost, h->stream));
        return VRC_OK;
    });
}

int vrc_box_intersection_device(vrc_caster *h, const void *d_boxes, int64_t n, int32_t max_voxels, uint32_t flags, void *d_records,
                                void *d_counts, void *d_voxels) {
    if (!h) return VRC_ERR_INVALID_ARGUMENT;
    int rc = box_check(h, d_boxes, n, max_voxels, flags, d_records, d_counts, d_voxels, "box_intersection_device");
    if (rc != VRC_OK || n == 0) return rc;
    return device_call(h, {{d_boxes, 3u}, {d_records, 3u}, {d_counts, 7u}, {d_voxels, 3u, max_voxels > 0}}, "box_intersection_device",
                       "boxes, records and voxels must be 4-byte aligned, counts 8-byte aligned", "boxes and outputs", [&] {
                           return box_enqueue(h, static_cast<const float *>(d_boxes), n, max_voxels, flags, static_cast<int32_t *>(d_records),
                                              static_cast<int64_t *>(d_counts), static_cast<int32_t *>(d_voxels));
                       });
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------------------------------------
// batched swept-box queries (vrc_sweep_boxes / vrc_sweep_boxes_device, box_sweep.hip)
// ---------------------------------------------------------------------------------------------------------------------------
namespace {

// the argument checks of both calls, then the readiness checks of the ray queries; nothing is launched when one fails
int sweep_check(vrc_caster *h, const void *sweeps, int64_t n, int32_t max_events, uint32_t flags, const void *records, const char *what) {
    if (n < 0) return fail(h, VRC_ERR_INVALID_ARGUMENT, "%s: n = %lld < 0", what, (long long)n);
    if (max_events < 0) return fail(h, VRC_ERR_INVALID_ARGUMENT, "%s: max_events = %d < 0", what, (int)max_events);
    VRC_TRY(flags_check(h, flags, VRC_SWEEP_STOPPING_ONLY, what));
    if (n > 0 && (!sweeps || !records)) return fail(h, VRC_ERR_INVALID_ARGUMENT, "%s: null sweeps or records", what);
    return query_check(h, sweeps, n, 0, 0, records, what);
}

// The shape flags and their scan, the start test (the box query's passes over the start boxes, a list of one voxel, into the
// handle's scratch), then the sweep kernels, on the handle's stream (current device: h->device).  The tree's guard is held
// throughout, as for a box query.  The one host wait is the start test's.
int sweep_enqueue(vrc_caster *h, const float *d_sweeps, int64_t n, int32_t max_events, uint32_t flags, int32_t *d_rec) {
    std::unique_lock<std::mutex> lock(h->tree->guard);
    VRC_TRY(grow(h, h->sweep_capacity, n, {{h->d_sweep_rec, sizeof(int32_t) * 8 * (size_t)n}, {h->d_sweep_vox, sizeof(int32_t) * 4 * (size_t)n},
                                           {h->d_sweep_cnt, sizeof(int64_t) * (size_t)n}, {h->d_sweep_scan, sizeof(int64_t) * 2 * (size_t)n}}));
    vrc::SweepParams p;
    memset(&p, 0, sizeof(p));
    vrc::BoxParams &q = p.box;
    q.boxes = d_sweeps; q.box_stride = 9; q.n = n; q.max_voxels = 1;
    q.flags = (flags & VRC_SWEEP_STOPPING_ONLY) ? vrc::kBoxStoppingOnly : 0u;
    q.records = h->d_sweep_rec; q.counts = h->d_sweep_cnt; q.voxels = h->d_sweep_vox;
    bind_scene(h, h->tree.get(), q.scene);
    p.records = d_rec;
    const int64_t dims = (int64_t)q.scene.map_dim[0] + q.scene.map_dim[1] + q.scene.map_dim[2];
    p.cap = max_events > 0 ? max_events : (int32_t)std::min<int64_t>(INT32_MAX, 2 * dims + 64);
    p.lane_face_max = (int32_t)std::max<int64_t>(0, std::min<int64_t>(INT32_MAX, setting_or(h, "sweep_lane_face", vrc::kSweepLaneFaceMax)));
    int64_t *big_cnt = h->d_sweep_scan, *big_end = h->d_sweep_scan + n;
    p.big_end = big_end;
    size_t need = 0;
    HIP_TRY(h, vrc::box_scan(nullptr, &need, big_cnt, big_end, n, h->stream));
    VRC_TRY(grow(h, h->box_temp_bytes, need, {{h->d_box_temp, need}}));
    HIP_TRY(h, vrc::launch_sweep_plan(p, big_cnt, h->stream));
    size_t bytes = h->box_temp_bytes;
    HIP_TRY(h, vrc::box_scan(h->d_box_temp, &bytes, big_cnt, big_end, n, h->stream));
    HIP_TRY(h, hipMemcpyAsync(&h->sweep_n_big, big_end + n - 1, sizeof(int64_t), hipMemcpyDeviceToHost, h->stream));
    VRC_TRY(box_passes(h, q));                                     // (waits for the stream: sweep_n_big has arrived)
    p.n_big = h->sweep_n_big;
    HIP_TRY(h, vrc::launch_sweep(p, h->stream));
    return VRC_OK;
}

}  // namespace

extern "C" {

int vrc_sweep_boxes(vrc_caster *h, const float *sweeps, int64_t n, int32_t max_events, uint32_t flags, int32_t *records) {
    if (!h) return VRC_ERR_INVALID_ARGUMENT;
    int rc = sweep_check(h, sweeps, n, max_events, flags, records, "sweep_boxes");
    if (rc != VRC_OK || n == 0) return rc;
    return host_call(h, [&]() -> int {
        VRC_TRY(grow(h, h->sweep_io_capacity, n, {{h->d_sweep_in, sizeof(float) * 9 * (size_t)n}, {h->d_sweep_out, sizeof(int32_t) * 8 * (size_t)n}}));
        HIP_TRY(h, hipMemcpyAsync(h->d_sweep_in, sweeps, sizeof(float) * 9 * (size_t)n, hipMemcpyHostToDevice, h->stream));
        VRC_TRY(sweep_enqueue(h, h->d_sweep_in, n, max_events, flags, h->d_sweep_out));
        HIP_TRY(h, hipMemcpyAsync(records, h->d_sweep_out, sizeof(int32_t) * 8 * (size_t)n, hipMemcpyDeviceToHost, h->stream));
        return VRC_OK;
    });
}

int vrc_sweep_boxes_device(vrc_caster *h, const void *d_sweeps, int64_t n, int32_t max_events, uint32_t flags, void *d_records) {
    if (!h) return VRC_ERR_INVALID_ARGUMENT;
    int rc = sweep_check(h, d_sweeps, n, max_events, flags, d_records, "sweep_boxes_device");
    if (rc != VRC_OK || n == 0) return rc;
    return device_call(h, {{d_sweeps, 3u}, {d_records, 3u}}, "sweep_boxes_device", "sweeps and records must be 4-byte aligned", "sweeps and records",
                       [&] { return sweep_enqueue(h, static_cast<const float *>(d_sweeps), n, max_events, flags, static_cast<int32_t *>(d_records)); });
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------------------------------------
// voxel reads (vrc_get_voxels / vrc_read_regions and their _device variants, voxel_read.hip)
// ---------------------------------------------------------------------------------------------------------------------------
namespace {

// the argument checks of the region reads, then the readiness checks of the ray queries; *total = n V, the bytes the call writes
int region_check(vrc_caster *h, const void *lo, int64_t n, const int32_t size[3], const void *out, size_t n_bytes, size_t *total, const char *what) {
    if (n < 0) return fail(h, VRC_ERR_INVALID_ARGUMENT, "%s: n = %lld < 0", what, (long long)n);
    VRC_TRY(size_check(h, size, what));
    if (n > 0 && (!lo || !out)) return fail(h, VRC_ERR_INVALID_ARGUMENT, "%s: null corners or output", what);
    VRC_TRY(volume_check(h, n, size, n_bytes, "output", nullptr, total, what));
    return query_check(h, lo, n, 0, 0, out, what);
}

// One launch on the handle's stream (current device: h->device): the points' values (size == nullptr) or the regions' bytes.
// The tree's guard is held until the kernel is enqueued, as box_enqueue holds it.
int read_enqueue(vrc_caster *h, const int32_t *d_in, int64_t n, const int32_t size[3], void *d_out) {
    std::unique_lock<std::mutex> lock(h->tree->guard);
    vrc::ReadParams q;
    memset(&q, 0, sizeof(q));
    q.positions = d_in; q.n = n;
    bind_scene(h, h->tree.get(), q.scene);
    if (!size) {
        q.values = static_cast<int32_t *>(d_out);
        HIP_TRY(h, vrc::launch_voxel_points(q, h->stream));
        return VRC_OK;
    }
    q.bytes = static_cast<int8_t *>(d_out);
    for (int a = 0; a < 3; a++) {
        q.size[a] = size[a];
        q.bricks[a] = bricks_along(size[a]);
    }
    // (n V fits size_t and a brick count is at most size + 1, so the wave count fits 64 bits with room to spare)
    HIP_TRY(h, vrc::launch_voxel_regions(q, h->stream));
    return VRC_OK;
}

// the host calls of both reads: positions or corners down, one launch, out_bytes of values or bytes up
int read_host(vrc_caster *h, const int32_t *in, int64_t n, const int32_t size[3], void *out, size_t out_bytes) {
    return host_call(h, [&]() -> int {
        VRC_TRY(grow(h, h->read_in_capacity, n, {{h->d_read_in, sizeof(int32_t) * 3 * (size_t)n}}));
        VRC_TRY(grow(h, h->read_out_bytes, out_bytes, {{h->d_read_out, out_bytes}}));
        HIP_TRY(h, hipMemcpyAsync(h->d_read_in, in, sizeof(int32_t) * 3 * (size_t)n, hipMemcpyHostToDevice, h->stream));
        VRC_TRY(read_enqueue(h, h->d_read_in, n, size, h->d_read_out));
        HIP_TRY(h, hipMemcpyAsync(out, h->d_read_out, out_bytes, hipMemcpyDeviceToHost, h->stream));
        return VRC_OK;
    });
}

// the _device calls of both reads (a region's bytes need no alignment)
int read_device(vrc_caster *h, const void *d_in, int64_t n, const int32_t size[3], void *d_out, const char *what) {
    return device_call(h, {{d_in, 3u}, {d_out, size ? 0u : 3u}}, what, size ? "the corners must be 4-byte aligned" : "positions and output must be 4-byte aligned",
                       "input and output", [&] { return read_enqueue(h, static_cast<const int32_t *>(d_in), n, size, d_out); });
}

}  // namespace

extern "C" {

int vrc_get_voxels(vrc_caster *h, const int32_t *positions, int64_t n, int32_t *out) {
    if (!h) return VRC_ERR_INVALID_ARGUMENT;
    int rc = query_check(h, positions, n, 0, 0, out, "get_voxels");
    if (rc != VRC_OK || n == 0) return rc;
    return read_host(h, positions, n, nullptr, out, sizeof(int32_t) * (size_t)n);
}

int vrc_get_voxels_device(vrc_caster *h, const void *d_positions, int64_t n, void *d_out) {
    if (!h) return VRC_ERR_INVALID_ARGUMENT;
    int rc = query_check(h, d_positions, n, 0, 0, d_out, "get_voxels_device");
    if (rc != VRC_OK || n == 0) return rc;
    return read_device(h, d_positions, n, nullptr, d_out, "get_voxels_device");
}

int vrc_read_regions(vrc_caster *h, const int32_t *lo, int64_t n, const int32_t size[3], int8_t *out, size_t n_bytes) {
    if (!h) return VRC_ERR_INVALID_ARGUMENT;
    size_t total = 0;
    int rc = region_check(h, lo, n, size, out, n_bytes, &total, "read_regions");
    if (rc != VRC_OK || n == 0) return rc;
    return read_host(h, lo, n, size, out, total);
}

int vrc_read_regions_device(vrc_caster *h, const void *d_lo, int64_t n, const int32_t size[3], void *d_out, size_t n_bytes) {
    if (!h) return VRC_ERR_INVALID_ARGUMENT;
    size_t total = 0;
    int rc = region_check(h, d_lo, n, size, d_out, n_bytes, &total, "read_regions_device");
    if (rc != VRC_OK || n == 0) return rc;
    return read_device(h, d_lo, n, size, d_out, "read_regions_device");
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------------------------------------
// exposed faces (vrc_extract_faces / vrc_extract_faces_device, face_extract.hip)
// ---------------------------------------------------------------------------------------------------------------------------
namespace {

// the argument checks of both calls, then the readiness checks of the ray queries; *items = n x the bricks a region can touch
int faces_check(vrc_caster *h, const void *lo, int64_t n, const int32_t size[3], int64_t capacity, uint32_t flags, const void *counts,
                const void *faces, const vrc_faces_info *info, int64_t *items, const char *what) {
    if (n < 0) return fail(h, VRC_ERR_INVALID_ARGUMENT, "%s: n = %lld < 0", what, (long long)n);
    VRC_TRY(size_check(h, size, what));
    if (capacity < 0) return fail(h, VRC_ERR_INVALID_ARGUMENT, "%s: capacity = %lld < 0", what, (long long)capacity);
    VRC_TRY(flags_check(h, flags, VRC_FACES_NO_MAP_EDGE | VRC_FACES_STOPPING_ONLY, what));
    if (n > 0 && (!lo || !counts)) return fail(h, VRC_ERR_INVALID_ARGUMENT, "%s: null corners or counts", what);
    if (n > 0 && capacity > 0 && !faces) return fail(h, VRC_ERR_INVALID_ARGUMENT, "%s: null faces with capacity = %lld", what, (long long)capacity);
    if (info && info->struct_size < sizeof(uint32_t)) return fail(h, VRC_ERR_INVALID_ARGUMENT, "%s: info->struct_size is not set", what);
    if ((uint64_t)capacity > SIZE_MAX / 16u) return fail(h, VRC_ERR_LIMIT, "%s: capacity * 16 bytes overflows size_t", what);
    // (axis by axis: a brick count is at most 2^28 + 1, so a product that passed the check times the next count fits 64 bits)
    uint64_t per = 1;
    for (int a = 0; a < 3; a++) {
        per *= (uint64_t)bricks_along(size[a]);
        if (per > (uint64_t)INT32_MAX) return fail(h, VRC_ERR_LIMIT, "%s: a region touches more than 2^31 - 1 bricks", what);
    }
    if (n > 0 && per > (uint64_t)INT32_MAX / (uint64_t)n) return fail(h, VRC_ERR_LIMIT, "%s: n * bricks per region exceeds 2^31 - 1", what);
    *items = (int64_t)per * n;
    return query_check(h, lo, n, 0, 0, counts, what);
}

// One extraction on the handle's stream (current device: h->device), in two timed segments with a host wait after each.  The
// tree's guard is held from faces_count to the end of the call, as box_enqueue holds it.
struct FaceCall {
    std::unique_lock<std::mutex> lock;
    vrc::FaceParams q;
    SegmentTimer timer;
    int64_t total = 0;
    double seconds = 0.0;
};

// count, scan, per-region counts; the grand total comes back in one 8-byte copy.  d_counts == nullptr: the counts go to the
// scratch behind the items' (the host call copies them out from c.q.counts)
int faces_count(vrc_caster *h, FaceCall &c, const int32_t *d_lo, int64_t n, const int32_t size[3], int64_t capacity, uint32_t flags,
                int64_t items, int64_t *d_counts) {
    c.lock = std::unique_lock<std::mutex>(h->tree->guard);
    vrc::FaceParams &q = c.q;
    memset(&q, 0, sizeof(q));
    q.lo = d_lo; q.n = n; q.flags = flags; q.capacity = capacity;
    for (int a = 0; a < 3; a++) {
        q.size[a] = size[a];
        q.bricks[a] = bricks_along(size[a]);
    }
    VRC_TRY(grow(h, h->face_item_capacity, 2 * items + n, {{h->d_face_items, sizeof(int64_t) * (size_t)(2 * items + n)}}));
    q.item_count = h->d_face_items; q.item_end = h->d_face_items + items;
    q.counts = d_counts ? d_counts : h->d_face_items + 2 * items;
    size_t need = 0;
    HIP_TRY(h, vrc::box_scan(nullptr, &need, q.item_count, q.item_end, items, h->stream));
    VRC_TRY(grow(h, h->box_temp_bytes, need, {{h->d_box_temp, need}}));
    bind_scene(h, h->tree.get(), q.scene);
    HIP_TRY(h, c.timer.init(h->stream, &c.seconds));
    HIP_TRY(h, c.timer.start());
    HIP_TRY(h, vrc::launch_face_count(q, h->stream));
    size_t bytes = h->box_temp_bytes;
    HIP_TRY(h, vrc::box_scan(h->d_box_temp, &bytes, q.item_count, q.item_end, items, h->stream));
    HIP_TRY(h, vrc::launch_face_regions(q, h->stream));
    HIP_TRY(h, c.timer.end(&c.total, q.item_end + items - 1, sizeof(int64_t)));
    return VRC_OK;
}

// the list, into d_faces (capacity entries); waits for the stream
int faces_emit(vrc_caster *h, FaceCall &c, int32_t *d_faces) {
    if (c.q.capacity > 0 && c.total > 0) {
        c.q.faces = d_faces;
        HIP_TRY(h, c.timer.start());
        HIP_TRY(h, vrc::launch_face_emit(c.q, h->stream));
        HIP_TRY(h, c.timer.end());
    }
    return VRC_OK;
}

void faces_report(vrc_faces_info *info, int64_t total, int64_t capacity, double seconds) {
    if (!info) return;
    vrc_faces_info out;
    memset(&out, 0, sizeof(out));
    out.truncated = total > capacity ? 1u : 0u;
    out.faces_total = total; out.faces_written = std::min(total, capacity); out.seconds = seconds;
    write_info(info, out);
}

}  // namespace

extern "C" {

int vrc_extract_faces(vrc_caster *h, const int32_t *lo, int64_t n, const int32_t size[3], int64_t capacity, uint32_t flags,
                      int64_t *counts, int32_t *faces, vrc_faces_info *info) {
    if (!h) return VRC_ERR_INVALID_ARGUMENT;
    int64_t items = 0;
    int rc = faces_check(h, lo, n, size, capacity, flags, counts, faces, info, &items, "extract_faces");
    if (rc != VRC_OK) return rc;
    if (n == 0) { faces_report(info, 0, capacity, 0.0); return VRC_OK; }
    FaceCall c;
    VRC_TRY(host_call(h, [&]() -> int {
        VRC_TRY(grow(h, h->read_in_capacity, n, {{h->d_read_in, sizeof(int32_t) * 3 * (size_t)n}}));
        HIP_TRY(h, hipMemcpyAsync(h->d_read_in, lo, sizeof(int32_t) * 3 * (size_t)n, hipMemcpyHostToDevice, h->stream));
        VRC_TRY(faces_count(h, c, h->d_read_in, n, size, capacity, flags, items, nullptr));
        HIP_TRY(h, hipMemcpyAsync(counts, c.q.counts, sizeof(int64_t) * (size_t)n, hipMemcpyDeviceToHost, h->stream));
        // the list is staged at the size it has, not at the size the caller made room for; only the written entries go back
        const size_t list_bytes = sizeof(int32_t) * 4 * (size_t)std::min(c.total, capacity);
        if (list_bytes) VRC_TRY(grow(h, h->read_out_bytes, list_bytes, {{h->d_read_out, list_bytes}}));
        c.q.capacity = std::min(c.total, capacity);
        VRC_TRY(faces_emit(h, c, static_cast<int32_t *>(h->d_read_out)));
        if (list_bytes) HIP_TRY(h, hipMemcpyAsync(faces, h->d_read_out, list_bytes, hipMemcpyDeviceToHost, h->stream));
        return VRC_OK;
    }));
    faces_report(info, c.total, capacity, c.seconds);
    return VRC_OK;
}

int vrc_extract_faces_device(vrc_caster *h, const void *d_lo, int64_t n, const int32_t size[3], int64_t capacity, uint32_t flags,
                             void *d_counts, void *d_faces, vrc_faces_info *info) {
    if (!h) return VRC_ERR_INVALID_ARGUMENT;
    int64_t items = 0;
    int rc = faces_check(h, d_lo, n, size, capacity, flags, d_counts, d_faces, info, &items, "extract_faces_device");
    if (rc != VRC_OK) return rc;
    if (n == 0) { faces_report(info, 0, capacity, 0.0); return VRC_OK; }
    FaceCall c;
    VRC_TRY(device_call(h, {{d_lo, 3u}, {d_counts, 7u}, {d_faces, 3u, capacity > 0}}, "extract_faces_device",
                        "the corners and faces must be 4-byte aligned, counts 8-byte aligned", "corners and outputs", [&]() -> int {
                            VRC_TRY(faces_count(h, c, static_cast<const int32_t *>(d_lo), n, size, capacity, flags, items, static_cast<int64_t *>(d_counts)));
                            return faces_emit(h, c, static_cast<int32_t *>(d_faces));
                        }));
    faces_report(info, c.total, capacity, c.seconds);
    return VRC_OK;
}

}  // extern "C"
